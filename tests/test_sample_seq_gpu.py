"""The sequence-aware draw on the device: xh_op_sample_seq against the reference
(tests/sample_seq_ref.py), xh_decode_sample_seq's loop against the adaptive loop, against a
teacher-forced replay, split in two (across the ring wrap too) and with graphs off, the top lists and
the timing hook."""
import ctypes

import numpy as np
import pytest

import constraint_ref as C
import sample_ext_ref as X
import sample_ref as R
import sample_seq_ref as Q
from conftest import fixture_path
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

FIXTURE = "tiny_mistral_f16"
# the prompt ends in a bigram it already holds (84 262, followed by 259): rep_259 = ng_259 = 2 at step 0
PROMPT = [1, 84, 262, 259, 90, 84, 262]
N = len(PROMPT)
EOS = 2
PATTERN = r"(of|to)( (of|to)){5}[.?]"
LOOP_CTL = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2, last_n=4)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_draws(an, out, case):
    """fired, kept rows, n_kept and tokens of every draw of one case against its analysis; returns
    the number of undecided draws."""
    undecided = open_draws = 0
    for i, tok in enumerate(out["tokens"].tolist()):
        pos = R.POS0 + i
        fired = an.fired(R.SEED, pos)
        assert bool(out["fired"][i]) == fired, (case, i)
        if not an.decided(fired):
            undecided += 1
            continue
        kept, final, n_kept = an.view(fired)
        assert np.array_equal(out["kept"][i], kept), (case, i, np.flatnonzero(out["kept"][i] != kept)[:8])
        assert int(out["n_kept"][i]) == n_kept, (case, i, int(out["n_kept"][i]), n_kept)
        ok = final.accepted(R.SEED, pos)
        open_draws += len(ok) != 1
        assert tok in ok and (len(ok) != 1 or tok == next(iter(ok))), (case, i, tok, ok)
    assert open_draws <= R.SKIP_CAP * len(out["tokens"]), (case, open_draws)
    return undecided


# ---- 1. op level: DRY and the ban, bit for bit -----------------------------------------------------
@pytest.mark.parametrize("V", Q.VOCABS)
def test_op_adjustment_grid_bitwise(V):
    lg = Q.logits(V)
    for n, kw in Q.dry_grid():
        kw = Q.grid_controls(V, kw)
        win = Q.grid_window(V, 1100)[:n]
        want, rep, ng = Q.seq_adjust(X.adjust(lg, win, **X.CTL_ON), win, **kw)
        out = L.op_sample_seq(lg, 0.0, 0, 1.0, R.SEED, R.POS0, 1, window=win, **X.CTL_ON, **kw)
        assert np.array_equal(out["rep"], rep) and np.array_equal(out["ng"], ng), (V, n, kw)
        assert np.array_equal(bits(out["adjusted"]), bits(want)), (V, n, kw)
        # temperature 0 with DRY and the ban: greedy over l', XTC takes no part
        assert out["tokens"].tolist() == [int(R.Analysis(want, 0.0, 0, 1.0).kept[0])] and not out["fired"].any()


@pytest.mark.parametrize("name", sorted(Q.edge_cases()))
def test_op_adjustment_edge_case(name):
    V, lg, win, seq, ctl, expect = Q.edge_cases()[name]
    want, rep, ng = Q.edge_expected(name)
    out = L.op_sample_seq(lg, 0.9, 0, 1.0, R.SEED, R.POS0, 8, window=win, xtc_probability=1.0, xtc_threshold=1.0, **ctl, **seq)
    assert np.array_equal(out["rep"], rep) and np.array_equal(out["ng"], ng), name
    assert np.array_equal(bits(out["adjusted"]), bits(want)), name
    if expect is not None:
        assert {int(c): (int(out["rep"][c]), int(out["ng"][c])) for c in np.flatnonzero(out["ng"])} == expect, name
    assert not np.isneginf(want[out["tokens"]]).any()
    greedy = L.op_sample_seq(lg, 0.0, 0, 1.0, R.SEED, R.POS0, 2, window=win, xtc_probability=1.0, **ctl, **seq)
    assert greedy["tokens"].tolist() == [int(R.Analysis(want, 0.0, 0, 1.0).kept[0])] * 2
    assert greedy["n_kept"].tolist() == [1, 1] and not greedy["fired"].any()


def test_op_bans_that_empty_the_vocabulary():
    lg, win, seq, ctl = Q.empty_vocabulary_case()
    for t in (0.0, 1.0):
        out = L.op_sample_seq(lg, t, 0, 1.0, R.SEED, R.POS0, 4, window=win, xtc_probability=1.0, **ctl, **seq)
        assert np.isneginf(out["adjusted"]).all()
        assert out["tokens"].tolist() == [0] * 4
        assert out["n_kept"].tolist() == ([0] * 4 if t else [1] * 4)


def test_op_dfa_mask_behind_the_ban():
    V = 300
    name = C.DFAS[0]
    nxt, acc = C.dfa(name)
    d = L.ByteDfa(nxt, acc)
    blob, offsets = L.pieces_blob(list(C.pieces(V)))
    lg = C.logits(V)
    state, stop = C.STATES[name][0]
    allowed, succ = C.mask(nxt, acc, C.pieces(V), state, stop)
    ok_ids = np.flatnonzero(allowed)
    assert ok_ids.size >= 3
    a = int(ok_ids[np.argmax(lg[ok_ids])])              # the constrained greedy choice, to be banned
    x = int(np.flatnonzero(~allowed.astype(bool))[0])
    win = [x, a, x]
    seq = dict(no_repeat_ngram=2, seq_last_n=8)
    l2, _, _ = Q.seq_adjust(lg, win, **seq)
    assert np.isneginf(l2[a])
    masked = C.masked_logits(l2, allowed, state)
    an = Q.SeqAnalysis(masked, 1.5)
    out = L.op_sample_seq(lg, 1.5, 0, 1.0, R.SEED, R.POS0, R.N_DRAWS, window=win, dfa=d, blob=blob, offsets=offsets,
                          state=state, stop=stop, **seq)
    assert np.array_equal(bits(out["adjusted"]), bits(l2))
    assert check_draws(an, out, name) == 0
    assert allowed[out["tokens"]].all() and a not in out["tokens"].tolist()
    assert out["states"].tolist() == [int(succ[t]) for t in out["tokens"].tolist()]
    greedy = L.op_sample_seq(lg, 0.0, 0, 1.0, R.SEED, R.POS0, 2, window=win, dfa=d, blob=blob, offsets=offsets, state=state,
                             stop=stop, **seq)
    assert greedy["tokens"].tolist() == [C.constrained_greedy(l2, allowed)] * 2 and a not in greedy["tokens"].tolist()


def test_op_xtc_under_a_dfa_mask_counts_the_masked_tokens():
    """C is every token (no top-k, min-p, n-sigma or typical stage), l'' holds -inf for what the DFA
    forbids: |C| = V in n_kept, the -inf entries stay in kept_out, none is in A or drawn."""
    V = 300
    name = C.DFAS[0]
    nxt, acc = C.dfa(name)
    d = L.ByteDfa(nxt, acc)
    blob, offsets = L.pieces_blob(list(C.pieces(V)))
    lg = C.logits(V)
    state, stop = C.STATES[name][0]
    allowed, succ = C.mask(nxt, acc, C.pieces(V), state, stop)
    masked = C.masked_logits(lg, allowed, state)
    an = Q.SeqAnalysis(masked, 3.0, xtc_probability=1.0, xtc_threshold=0.002)
    assert an.decided(True) and 2 <= an.n_a < int(allowed.sum())
    out = L.op_sample_seq(lg, 3.0, 0, 1.0, R.SEED, R.POS0, R.N_DRAWS, dfa=d, blob=blob, offsets=offsets, state=state,
                          stop=stop, xtc_probability=1.0, xtc_threshold=0.002)
    assert check_draws(an, out, name) == 0 and out["fired"].all()
    assert out["n_kept"].tolist() == [V - (an.n_a - 1)] * R.N_DRAWS
    assert out["kept"][0][~allowed.astype(bool)].all() and int(out["kept"][0].sum()) == V - (an.n_a - 1)
    assert allowed[out["tokens"]].all()


# ---- 2. op level: XTC --------------------------------------------------------------------------------
@pytest.mark.parametrize("V", Q.VOCABS)
def test_op_xtc_grid_matches_reference(V):
    lg = Q.logits(V)
    skipped = 0
    for case in Q.xtc_grid():
        t, k, ty, p, pr, th = case
        an = Q.xtc_analysis(V, *case)
        if not (an.decided(True) and an.decided(False)):
            skipped += 1
            continue
        out = L.op_sample_seq(lg, t, k, p, R.SEED, R.POS0, R.N_DRAWS, typical_p=ty, xtc_probability=pr, xtc_threshold=th)
        assert check_draws(an, out, (V,) + case) == 0
        assert np.array_equal(bits(out["adjusted"]), bits(lg))
    assert skipped <= R.SKIP_CAP * len(Q.xtc_grid())


@pytest.mark.parametrize("name", sorted(Q.xtc_edge_cases()))
def test_op_xtc_edge_case(name):
    lg, kw, n_a, kept_ids = Q.xtc_edge_cases()[name]
    an = Q.xtc_edge_analysis(name)
    assert an.decided(True) and an.decided(False), (name, an.reasons, an.off.reasons)
    out = L.op_sample_seq(lg, kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), R.SEED, R.POS0, R.N_DRAWS,
                          typical_p=kw.get("typical_p", 1.0), xtc_probability=kw["xtc_probability"],
                          xtc_threshold=kw["xtc_threshold"])
    assert check_draws(an, out, name) == 0
    if kw["xtc_probability"] == 1.0:
        assert out["fired"].all()
        if kept_ids is not None:
            assert np.flatnonzero(out["kept"][0]).tolist() == kept_ids
    else:
        assert 0 < int(out["fired"].sum()) < R.N_DRAWS


# ---- the loop on the fixture -------------------------------------------------------------------------
def fixture_pieces():
    return L.token_pieces(XalmFile(fixture_path(FIXTURE + ".xalm")).tokens())


def hydrated(graphs=True, constraint=False, fixture=FIXTURE, prompt=PROMPT):
    gm = Model.from_xalm(XalmFile(fixture_path(fixture + ".xalm")))
    gm.set_graphs(graphs)
    dfa = L.regex_compile(PATTERN)
    if constraint:
        gm.set_constraint_vocab(fixture_pieces())
        gm.set_constraint(dfa)
    st = InferenceState(gm.config)
    for pos, tok in enumerate(prompt):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    return gm, st, dfa


# ---- 3. everything off: the adaptive loop, bit for bit -----------------------------------------------------
@pytest.mark.parametrize("graphs", (True, False))
@pytest.mark.parametrize("fixture", (FIXTURE, "tiny_mistral_q4_0"))
def test_loop_with_everything_off_is_the_adaptive_loop(graphs, fixture):
    ctl = dict(LOOP_CTL, min_p=0.02)
    for kw in (dict(temperature=0.0), dict(temperature=0.9, top_k=40, top_p=0.95, typical_p=0.9, top_n_sigma=2.0),
               dict(temperature=1.2, mirostat_tau=3.0, mirostat_eta=0.2)):
        kw = dict(kw, seed=7, history=PROMPT, state=5, **(ctl if "mirostat_tau" not in kw else LOOP_CTL))
        gm, _, _ = hydrated(graphs, fixture=fixture)
        want = gm.decode_sample_adapt(N, 24, **kw)
        gm.close()
        gm, _, _ = hydrated(graphs, fixture=fixture)
        got = gm.decode_sample_seq(N, 24, seq_last_n=64, **kw)      # a window alone switches nothing on
        gm.close()
        assert got[0] == want[0] and bits(got[1]).tolist() == bits(want[1]).tolist(), kw
        assert got[2] == want[2] == 5 and bits([got[3]])[0] == bits([want[3]])[0], kw


@pytest.mark.parametrize("graphs", (True, False))
def test_loop_with_everything_off_is_the_constrained_adaptive_loop(graphs):
    kw = dict(top_k=40, top_p=0.95, typical_p=0.9, seed=5, constrain=True, history=PROMPT, stop=(EOS, -1), min_p=0.02, **LOOP_CTL)
    for t in (0.0, 1.1):
        gm, _, dfa = hydrated(graphs, constraint=True)
        want = gm.decode_sample_adapt(N, 24, t, state=dfa.start, **kw)
        gm.close()
        gm, _, _ = hydrated(graphs, constraint=True)
        got = gm.decode_sample_seq(N, 24, t, state=dfa.start, **kw)
        gm.close()
        assert got[0] == want[0] and got[2] == want[2] and bits(got[1]).tolist() == bits(want[1]).tolist(), t
        assert got[0][-1] == EOS


# ---- 4. the loop against a teacher-forced replay ----------------------------------------------------------
SEQ = dict(dry_multiplier=0.8, dry_base=1.75, dry_allowed_length=2, no_repeat_ngram=3, seq_last_n=1024, breakers=(90, 7),
           xtc_probability=0.5, xtc_threshold=0.02)
STEPS = 48
SETTINGS = {"greedy": dict(temperature=0.0, seed=3), "sampled": dict(temperature=1.1, top_k=20, seed=9)}


def seq_run(setting, graphs=True, split=None, steps=STEPS, prompt=PROMPT, history=None):
    kw = dict(SETTINGS[setting], **LOOP_CTL, **SEQ)
    hist = list(prompt if history is None else history)
    gm, _, _ = hydrated(graphs, prompt=prompt)
    toks, lps, _, _ = gm.decode_sample_seq(len(prompt), split or steps, history=hist, **kw)
    if split:
        b, lb, _, _ = gm.decode_sample_seq(len(prompt) + split, steps - split, history=hist + toks, **kw)
        toks, lps = toks + b, np.concatenate([lps, lb])
    gm.close()
    return toks, lps


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_loop_against_replay(setting):
    toks, lps = seq_run(setting)
    assert len(toks) == STEPS
    s = SETTINGS[setting]
    t, seed, k = s["temperature"], s["seed"], s.get("top_k", 0)
    gm, st, _ = hydrated()
    hist, undecided, open_draws, n_dry, n_ban, n_xtc = list(PROMPT), 0, 0, 0, 0, 0
    for i, tok in enumerate(toks):
        raw = st.logits().copy()
        lp = X.adjust(raw, hist, **LOOP_CTL)
        l2, rep, ng = Q.seq_adjust(lp, hist, **SEQ)
        n_dry += bool((rep >= SEQ["dry_allowed_length"]).any())
        n_ban += bool((ng >= SEQ["no_repeat_ngram"] - 1).any())
        if t == 0.0:
            assert tok == int(R.Analysis(l2, 0.0, 0, 1.0).kept[0]), i
        else:
            an = Q.SeqAnalysis(l2, t, xtc_probability=SEQ["xtc_probability"], xtc_threshold=SEQ["xtc_threshold"], top_k=k)
            fired = an.fired(seed, N + i)
            if an.decided(fired):
                n_xtc += fired and an.n_a >= 2
                ok = an.view(fired)[1].accepted(seed, N + i)
                open_draws += len(ok) != 1
                assert tok in ok and (len(ok) != 1 or tok == next(iter(ok))), (i, tok, ok)
            else:
                undecided += 1
        want_lp = X.logprob64(raw, tok)
        assert abs(float(lps[i]) - want_lp) <= X.logprob_bound(want_lp), i
        hist.append(tok)
        if i + 1 < len(toks):
            gm.forward(st, tok, N + i, L.OUTPUT_LOGITS)
    gm.close()
    assert undecided <= R.SKIP_CAP * STEPS and open_draws <= R.SKIP_CAP * STEPS
    assert n_dry >= 1 and n_ban >= 1 and (t == 0.0 or n_xtc >= 1), (n_dry, n_ban, n_xtc)
    # one call equals two at splits 1, 17 and n - 1; graphs on equals graphs off
    for graphs, split in ((False, None), (True, 1), (True, 17), (False, 17), (True, STEPS - 1)):
        t2, l2 = seq_run(setting, graphs, split)
        assert t2 == toks and bits(l2).tolist() == bits(lps).tolist(), (graphs, split)


def test_one_call_equals_two_across_the_ring_wrap():
    """n_history = 1010 and 40 steps: the ring's count passes 1024 inside the run."""
    rng = np.random.default_rng(77)
    pre = [int(t) for t in rng.integers(3, 200, 1010 - N)]
    pre[-40:-20] = pre[-20:]               # a repeat inside the history the matches can reach
    history = pre + PROMPT
    assert len(history) == 1010
    runs = [seq_run("sampled", True, split, steps=40, history=history) for split in (None, 14, 20)]
    runs.append(seq_run("sampled", False, None, steps=40, history=history))
    for toks, lps in runs[1:]:
        assert toks == runs[0][0] and bits(lps).tolist() == bits(runs[0][1]).tolist()
    assert len(runs[0][0]) == 40


# ---- 5. top lists and the timing hook ---------------------------------------------------------------------
def test_top_lists_and_timing_hook():
    gm, st, _ = hydrated()
    us = ctypes.c_float(0)
    assert L.lib().xh_time_kernel(gm._ctx, 11, 4, ctypes.byref(us)) == 3   # XH_E_STATE before any call
    gm.set_top_logprobs(4)
    raw = st.logits().copy()
    toks, lps, _, _ = gm.decode_sample_seq(N, 6, history=PROMPT, **SETTINGS["sampled"], **SEQ)
    ids, tl, rank = gm.top_logprobs(6)
    assert ids.shape == (6, 4) and int(ids[0, 0]) == int(np.argmax(raw))
    for i, tok in enumerate(toks):
        if rank[i] < 4:
            assert int(ids[i, rank[i]]) == tok and bits([tl[i, rank[i]]])[0] == bits([lps[i]])[0]
    assert gm.time_kernel(11, 4) > 0.0 and gm.time_kernel(10, 4) > 0.0
    gm.close()


def test_mirostat_with_xtc_is_rejected():
    gm, _, _ = hydrated()
    with pytest.raises(L.XhError, match="xtc_probability"):
        gm.decode_sample_seq(N, 4, 1.0, mirostat_tau=3.0, xtc_probability=0.5, history=PROMPT)
    gm.close()


# ---- 6. the CLI -----------------------------------------------------------------------------------------
def cli(*args):
    import os
    import re
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "xalm_amd", "bin", "xalm")
    r = subprocess.run([exe, fixture_path(FIXTURE + ".xalm"), "-n", "16", "-i", "the answer is the answer is", *args],
                       capture_output=True, timeout=120)
    out = r.stdout.decode("utf-8", errors="replace")
    ids = re.search(r"tokens: \[([0-9,]*)\]", out)
    return r.returncode, [int(v) for v in ids.group(1).split(",")] if ids else None, r.stderr.decode(errors="replace")


@pytest.mark.parametrize("flags", [("-t", "0", "-D", "0.8", "-B", "1.75", "-A", "2", "-N", "3", "-W", "64"),
                                   ("-t", "1.1", "-k", "20", "-s", "9", "-D", "0.8", "-N", "3", "-X", "0.5", "-x", "0.02"),
                                   ("-t", "1.0", "-s", "4", "-y", "0.9", "-X", "1.0", "-x", "0.05", "-r", "1.3", "-w", "8")])
def test_cli_host_and_device_routes_agree(flags):
    runs = {}
    for g in ("0", "1"):
        rc, ids, err = cli("-g", g, *flags)
        assert rc == 0, err
        runs[g] = ids
    assert runs["0"] == runs["1"] and len(runs["1"]) > 4


def test_cli_rejects_mirostat_with_xtc():
    for g in ("0", "1"):
        rc, ids, err = cli("-g", g, "-t", "1.0", "-U", "3.0", "-X", "0.5")
        assert rc != 0 and ids is None and "xtc_probability" in err, (g, err)
