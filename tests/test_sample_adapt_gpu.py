"""The adaptive draw on the device: xh_op_sample_adapt against the reference (tests/sample_adapt_ref.py),
xh_decode_sample_adapt's loop against the older loops, against a teacher-forced replay, split in two
and with graphs off, the top lists, the timing hook and the CLI's two routes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import constraint_ref as C
import sample_adapt_ref as A
import sample_ext_ref as X
import sample_ref as R
from conftest import ROOT, fixture_path
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

FIXTURE = "tiny_mistral_f16"
PROMPT = [1, 84, 262, 259, 90]
N = len(PROMPT)
EOS = 2
PATTERN = r"(of|to)( (of|to)){5}[.?]"   # test_constraint_gpu.py's: at most 19 tokens with the end token
LOOP_CTL = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2, last_n=4)
CLI = os.path.join(ROOT, "xalm_amd", "bin", "xalm")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_draws(an, out, case, lg_adj):
    """tokens, n_kept, kept_out and thr_out of one decided case against its analysis."""
    assert np.array_equal(out["kept"], an.kept_map), (case, np.flatnonzero(out["kept"] != an.kept_map)[:8])
    assert (out["n_kept"] == an.n_kept).all(), (case, out["n_kept"][:4], an.n_kept)
    if np.isfinite(an.thr):
        assert abs(out["thr"] - an.thr) <= float(np.spacing(np.float32(abs(an.thr)))), (case, out["thr"], an.thr)
    else:
        assert out["thr"] == an.thr, case
    open_draws = 0
    for i, tok in enumerate(out["tokens"].tolist()):
        ok = an.accepted(R.SEED, R.POS0 + i)
        open_draws += len(ok) != 1
        assert tok in ok and (len(ok) != 1 or tok == next(iter(ok))), (case, i, tok, ok)
        if an.K is not None:
            want, obs = an.mu_next(tok)
            assert abs(float(out["mu"][i]) - want) <= A.mu_bound(an.mu, obs, an.tau), (case, i, float(out["mu"][i]), want)
        else:
            assert float(out["mu"][i]) == an.mu
    assert open_draws <= R.SKIP_CAP * len(out["tokens"]), (case, open_draws)


# ---- 1. the grids --------------------------------------------------------------------------------
@pytest.mark.parametrize("V", A.VOCABS)
def test_op_grid_matches_reference(V):
    lg = R.peaked_logits(V)
    skipped = 0
    for (t, k, ty, ns, p) in A.grid():
        an = A.grid_analysis(V, t, k, ty, ns, p)
        if not an.decided:
            skipped += 1
            continue
        out = L.op_sample_adapt(lg, t, k, p, R.SEED, R.POS0, R.N_DRAWS, typical_p=ty, top_n_sigma=ns)
        check_draws(an, out, (V, t, k, ty, ns, p), lg)
    assert skipped <= R.SKIP_CAP * len(A.grid())


@pytest.mark.parametrize("V", A.VOCABS)
def test_op_mirostat_grid_matches_reference(V):
    lg = R.peaked_logits(V)
    for (t, tau, eta, mu) in A.miro_grid():
        an = A.miro_analysis(V, t, tau, eta, mu)
        if not an.decided:
            continue
        out = L.op_sample_adapt(lg, t, 0, 1.0, R.SEED, R.POS0, R.N_DRAWS, mirostat_tau=tau, mirostat_eta=eta, mu=mu)
        check_draws(an, out, (V, t, tau, eta, mu), lg)


# ---- 2. the edge cases ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(A.edge_cases()))
def test_op_edge_case(name):
    lg, kw, ctl, kept = A.edge_cases()[name]
    an = A.edge_analysis(name)
    assert an.decided, (name, an.reasons)
    out = L.op_sample_adapt(lg, kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), R.SEED, R.POS0, R.N_DRAWS,
                            typical_p=kw.get("typical_p", 1.0), top_n_sigma=kw.get("top_n_sigma", 0.0),
                            mirostat_tau=kw.get("tau", 0.0), mirostat_eta=kw.get("eta", 0.1), mu=kw.get("mu", 0.0),
                            min_p=kw.get("min_p", 0.0), **ctl)
    check_draws(an, out, name, X.adjust(lg, (), **ctl))
    if kept is not None:
        assert np.flatnonzero(out["kept"]).tolist() == kept
    if ctl:
        assert not set(out["tokens"].tolist()) & {t for t, _ in A.BAN}


def test_op_dfa_mask_in_front_of_typical():
    V = 300
    name = C.DFAS[0]
    nxt, acc = C.dfa(name)
    d = L.ByteDfa(nxt, acc)
    blob, offsets = L.pieces_blob(list(C.pieces(V)))
    lg = C.logits(V)
    state, stop = C.STATES[name][0]
    allowed, succ = C.mask(nxt, acc, C.pieces(V), state, stop)
    masked = C.masked_logits(lg, allowed, state)
    assert 2 <= allowed.sum() < V
    for ty, ns in ((0.5, 0.0), (0.9, 1.0)):
        an = A.AdaptAnalysis(masked, 1.5, typical_p=ty, top_n_sigma=ns)
        assert an.decided, an.reasons
        out = L.op_sample_adapt(lg, 1.5, 0, 1.0, R.SEED, R.POS0, R.N_DRAWS, typical_p=ty, top_n_sigma=ns, dfa=d, blob=blob,
                                offsets=offsets, state=state, stop=stop)
        check_draws(an, out, (name, ty, ns), masked)
        assert allowed[out["tokens"]].all()
        assert out["states"].tolist() == [int(succ[t]) for t in out["tokens"].tolist()]
    # temperature 0: the constrained greedy choice, the truncation ignored
    out = L.op_sample_adapt(lg, 0.0, 0, 1.0, R.SEED, R.POS0, 4, typical_p=0.2, top_n_sigma=1.0, dfa=d, blob=blob,
                            offsets=offsets, state=state, stop=stop)
    assert out["tokens"].tolist() == [C.constrained_greedy(lg, allowed)] * 4 and out["n_kept"].tolist() == [1] * 4


# ---- the loop on the fixture -------------------------------------------------------------------------
def fixture_pieces():
    return L.token_pieces(XalmFile(fixture_path(FIXTURE + ".xalm")).tokens())


def hydrated(graphs=True, constraint=False, fixture=FIXTURE):
    gm = Model.from_xalm(XalmFile(fixture_path(fixture + ".xalm")))
    gm.set_graphs(graphs)
    dfa = L.regex_compile(PATTERN)
    if constraint:
        gm.set_constraint_vocab(fixture_pieces())
        gm.set_constraint(dfa)
    st = InferenceState(gm.config)
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    return gm, st, dfa


# ---- 3. equivalence with the older loops ----------------------------------------------------------------
@pytest.mark.parametrize("graphs", (True, False))
@pytest.mark.parametrize("fixture", (FIXTURE, "small_llama_f16"))
def test_loop_with_everything_off_is_the_extended_loop(graphs, fixture):
    ctl = dict(LOOP_CTL, min_p=0.02)
    for t, k, p in ((0.0, 0, 1.0), (0.9, 40, 0.95), (1.3, 0, 1.0)):
        gm, _, _ = hydrated(graphs, fixture=fixture)
        want, wl = gm.decode_sample_ext(N, 24, t, k, p, 7, history=PROMPT, logprobs=True, **ctl)
        gm.close()
        gm, _, _ = hydrated(graphs, fixture=fixture)
        toks, lps, state, mu = gm.decode_sample_adapt(N, 24, t, k, p, 7, history=PROMPT, state=5, **ctl)
        gm.close()
        assert toks == want and bits(lps).tolist() == bits(wl).tolist(), (t, k, p)
        assert state == 5 and mu == 0.0


@pytest.mark.parametrize("graphs", (True, False))
def test_loop_with_everything_off_is_the_constrained_loop(graphs):
    ctl = dict(LOOP_CTL, min_p=0.02)
    for t, k, p in ((0.0, 0, 1.0), (1.1, 40, 0.95)):
        gm, _, dfa = hydrated(graphs, constraint=True)
        want, wl, ws = gm.decode_sample_dfa(N, 24, t, dfa.start, k, p, 5, history=PROMPT, stop=(EOS, -1), **ctl)
        gm.close()
        gm, _, _ = hydrated(graphs, constraint=True)
        toks, lps, state, _ = gm.decode_sample_adapt(N, 24, t, k, p, 5, constrain=True, state=dfa.start, history=PROMPT,
                                                     stop=(EOS, -1), **ctl)
        gm.close()
        assert toks == want and state == ws and bits(lps).tolist() == bits(wl).tolist(), (t, k, p)
        assert toks[-1] == EOS


# ---- 4. the Mirostat loop ------------------------------------------------------------------------------
MIRO = dict(mirostat_tau=3.0, mirostat_eta=0.2)
MIRO_T, MIRO_SEED, MIRO_STEPS = 1.2, 9, 48


def miro_run(graphs, split=None):
    gm, _, _ = hydrated(graphs)
    toks, lps, _, mu = gm.decode_sample_adapt(N, split or MIRO_STEPS, MIRO_T, seed=MIRO_SEED, history=PROMPT, **LOOP_CTL, **MIRO)
    if split:
        b, lb, _, mu = gm.decode_sample_adapt(N + split, MIRO_STEPS - split, MIRO_T, seed=MIRO_SEED, mu=mu,
                                              history=PROMPT + toks, **LOOP_CTL, **MIRO)
        toks, lps = toks + b, np.concatenate([lps, lb])
    gm.close()
    return toks, lps, mu


def test_mirostat_loop_against_replay():
    toks, lps, mu_end = miro_run(True)
    assert len(toks) == MIRO_STEPS
    # the mu after every token: calls of one step each on a second context, mu carried
    gm, _, _ = hydrated()
    mus, mu = [], 2.0 * MIRO["mirostat_tau"]
    for i in range(MIRO_STEPS):
        one, _, _, mu = gm.decode_sample_adapt(N + i, 1, MIRO_T, seed=MIRO_SEED, mu=mu, history=PROMPT + toks[:i],
                                               **LOOP_CTL, **MIRO)
        assert one == [toks[i]], (i, one, toks[i])
        mus.append(mu)
    gm.close()
    assert bits([mus[-1]])[0] == bits([mu_end])[0]
    assert len(set(mus)) > MIRO_STEPS // 2   # the controller moves
    # teacher-forced: the reference on exactly the logits of every step, re-anchored to the device's mu
    gm, st, _ = hydrated()
    hist, mu, open_draws, undecided = list(PROMPT), 2.0 * MIRO["mirostat_tau"], 0, 0
    for i, tok in enumerate(toks):
        raw = st.logits().copy()
        an = A.AdaptAnalysis(X.adjust(raw, hist, **LOOP_CTL), MIRO_T, tau=MIRO["mirostat_tau"], eta=MIRO["mirostat_eta"], mu=mu)
        if an.decided:
            ok = an.accepted(MIRO_SEED, N + i)
            open_draws += len(ok) != 1
            assert tok in ok and (len(ok) != 1 or tok == next(iter(ok))), (i, tok, ok)
            want, obs = an.mu_next(tok)
            assert abs(mus[i] - want) <= A.mu_bound(mu, obs, an.tau), (i, mus[i], want)
        else:
            undecided += 1
        want_lp = X.logprob64(raw, tok)
        assert abs(float(lps[i]) - want_lp) <= X.logprob_bound(want_lp), i
        mu = mus[i]
        hist.append(tok)
        if i + 1 < len(toks):
            gm.forward(st, tok, N + i, L.OUTPUT_LOGITS)
    gm.close()
    assert undecided <= R.SKIP_CAP * MIRO_STEPS and open_draws <= R.SKIP_CAP * MIRO_STEPS
    # one call equals 17 + 31, graphs on equals graphs off: tokens, logprob bits and the bits of mu
    for graphs, split in ((False, None), (True, 17), (False, 17)):
        t2, l2, m2 = miro_run(graphs, split)
        assert t2 == toks and bits([m2])[0] == bits([mu_end])[0] and bits(l2).tolist() == bits(lps).tolist(), (graphs, split)


# ---- 5. typical + n-sigma under penalties and a regex ---------------------------------------------------
def test_typical_n_sigma_loop_one_call_equals_two():
    kw = dict(typical_p=0.9, top_n_sigma=2.0, top_p=0.95, seed=5, constrain=True, stop=(EOS, -1), **LOOP_CTL)
    runs = []
    for graphs, split in ((True, None), (True, 7), (False, None)):
        gm, _, dfa = hydrated(graphs, constraint=True)
        toks, lps, state, _ = gm.decode_sample_adapt(N, split or 24, 1.1, state=dfa.start, history=PROMPT, **kw)
        if split and len(toks) == split and toks[-1] != EOS:
            b, lb, state, _ = gm.decode_sample_adapt(N + split, 24 - split, 1.1, state=state, history=PROMPT + toks, **kw)
            toks, lps = toks + b, np.concatenate([lps, lb])
        gm.close()
        runs.append((toks, state, bits(lps).tolist()))
    assert runs[0] == runs[1] == runs[2]
    toks, state, _ = runs[0]
    assert len(toks) > 7 and toks[-1] == EOS and dfa.accept[state]
    text = b"".join(fixture_pieces()[t] for t in toks[:-1])
    assert re.fullmatch(PATTERN.encode(), text), text


# ---- 6. top lists, 7. the timing hook -------------------------------------------------------------------
def test_top_lists_and_timing_hook():
    gm, st, _ = hydrated()
    us = ctypes.c_float(0)
    assert L.lib().xh_time_kernel(gm._ctx, 10, 4, ctypes.byref(us)) == 3   # XH_E_STATE before any call
    gm.set_top_logprobs(4)
    raw = st.logits().copy()
    toks, lps, _, _ = gm.decode_sample_adapt(N, 6, 1.1, seed=3, typical_p=0.9, top_n_sigma=2.0, history=PROMPT)
    ids, tl, rank = gm.top_logprobs(6)
    assert ids.shape == (6, 4) and int(ids[0, 0]) == int(np.argmax(raw))
    for i, tok in enumerate(toks):
        if rank[i] < 4:
            assert int(ids[i, rank[i]]) == tok and bits([tl[i, rank[i]]])[0] == bits([lps[i]])[0]
    assert gm.time_kernel(10, 4) > 0.0
    gm.close()


# ---- 8. the CLI ------------------------------------------------------------------------------------
def cli(*args):
    r = subprocess.run([CLI, fixture_path(FIXTURE + ".xalm"), "-n", "16", "-i", "the answer is", *args], capture_output=True,
                       timeout=120)
    out = r.stdout.decode("utf-8", errors="replace")
    ids = re.search(r"tokens: \[([0-9,]*)\]", out)
    return r.returncode, [int(v) for v in ids.group(1).split(",")] if ids else None, r.stderr.decode(errors="replace")


@pytest.mark.parametrize("flags", [("-t", "1.1", "-y", "0.9", "-s", "11"), ("-t", "1.1", "-S", "1.5", "-p", "0.95", "-s", "4"),
                                   ("-t", "1.2", "-U", "3.0", "-E", "0.2", "-s", "7", "-r", "1.3", "-w", "8")])
def test_cli_host_and_device_routes_agree(flags):
    runs = {}
    for g in ("0", "1"):
        rc, ids, err = cli("-g", g, *flags)
        assert rc == 0, err
        runs[g] = ids
    assert runs["0"] == runs["1"] and len(runs["1"]) > 4


def test_cli_rejects_mirostat_with_top_k():
    rc, ids, err = cli("-g", "1", "-t", "1.0", "-U", "3.0", "-k", "40")
    assert rc != 0 and ids is None and "xh_decode_sample_adapt" in err
