"""The extended draw on the device: xh_op_sample_ext against the numpy reference
(tests/sample_ext_ref.py) and xh_decode_sample_ext's loop on two tiny fixtures of different weight
type."""
import os
import re
import subprocess

import numpy as np
import pytest

import sample_ext_ref as X
import sample_ref as R
from conftest import ROOT, fixture_path
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "xalm_amd", "bin", "xalm")
FIXTURES = ["tiny_mistral_f16", "tiny_mistral_f8_e4m3"]
PROMPT = [1, 84, 262, 259, 90]
N = len(PROMPT)
# the loop's controls: a window of 4, so tokens leave it during 30 steps
LOOP_CTL = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2, last_n=4)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the op ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", X.ADJ_VOCABS)
def test_adjusted_logits_bit_for_bit(V):
    lg = X.adjust_logits_vector(V)
    for name, (win, ctl) in X.adjust_cases(V).items():
        want = X.adjust(lg, win, **ctl)
        _, _, got, _ = L.op_sample_ext(lg, 0.0, 0, 1.0, 1, 0, 1, window=win, **ctl)
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("V", R.VOCABS)
def test_draws_match_reference(V):
    lg = R.peaked_logits(V)
    grid = X.draw_grid()
    skipped = 0
    for (t, k, p, mp, on) in grid:
        an = X.draw_analysis(V, t, k, p, mp, on)
        ctl = dict(X.CTL_ON) if on else {}
        toks, kept, adj, _ = L.op_sample_ext(lg, t, k, p, R.SEED, R.POS0, R.N_DRAWS, window=X.draw_window(V) if on else (),
                                             min_p=mp, **ctl)
        assert (bits(adj) == bits(X.draw_adjusted(V, on))).all(), (t, k, p, mp, on)
        if not an.decided:
            skipped += 1
            continue
        assert (kept == an.n_kept).all(), (t, k, p, mp, on, kept[:4], an.n_kept)
        for d in range(R.N_DRAWS):
            assert int(toks[d]) in an.accepted(R.SEED, R.POS0 + d), (t, k, p, mp, on, d, int(toks[d]))
        if mp == 1.0:  # exactly the maxima of l'
            mx = np.flatnonzero(X.draw_adjusted(V, on) == X.draw_adjusted(V, on).max())
            assert an.n_kept == min(mx.size, k or V) and set(toks.tolist()) <= set(mx.tolist())
    assert skipped <= R.SKIP_CAP * len(grid)


@pytest.mark.parametrize("name", sorted(X.edge_cases()))
def test_edge_cases(name):
    lg, win, t, k, p, ctl, kept_ids = X.edge_cases()[name]
    an = X.edge_analysis(name)
    assert an.decided
    toks, kept, adj, _ = L.op_sample_ext(lg, t, k, p, R.SEED, R.POS0, R.N_DRAWS, window=win, **ctl)
    assert (bits(adj) == bits(X.adjust(lg, win, **ctl))).all()
    assert (kept == an.n_kept).all(), (kept[:4], an.n_kept)
    for d in range(R.N_DRAWS):
        assert int(toks[d]) in an.accepted(R.SEED, R.POS0 + d), (d, int(toks[d]))
    if kept_ids is not None:
        assert set(toks.tolist()) <= set(kept_ids)
    if name == "greedy_demoted":  # the argmax of l', not of l
        assert set(toks.tolist()) == {41} and int(np.argmax(lg)) == 40
    if name == "ban_argmax":
        assert 40 not in toks.tolist() and int(np.argmax(lg)) == 40
    if name.startswith("min_p_1"):  # 64 draws over two or three tokens of equal weight reach each
        assert set(toks.tolist()) == set(kept_ids)


@pytest.mark.parametrize("V", (300, 128256))
def test_identity_with_controls_off(V):
    lg = R.peaked_logits(V)
    win = X.draw_window(V)
    for (t, k, p) in ((0.7, 40, 0.9), (1.5, 0, 1.0), (0.0, 0, 1.0)):
        want, want_kept = L.op_sample(lg, t, k, p, R.SEED, R.POS0, R.N_DRAWS)
        for window, ctl in (((), {}), (win, {}), (win, dict(last_n=0)), (win, dict(last_n=64))):
            toks, kept, adj, _ = L.op_sample_ext(lg, t, k, p, R.SEED, R.POS0, R.N_DRAWS, window=window, **ctl)
            assert toks.tolist() == want.tolist() and kept.tolist() == want_kept.tolist()
            assert (bits(adj) == bits(lg)).all()
    # a null ctl pointer
    import ctypes
    s = L.XhSampling(0.7, 40, 0.9, R.SEED)
    toks = np.empty(R.N_DRAWS, np.int32)
    kept = np.empty(R.N_DRAWS, np.int32)
    L.check(L.lib().xh_op_sample_ext(L.ptr(lg), V, ctypes.byref(s), None, None, 0, R.POS0, R.N_DRAWS, L.ptr(toks),
                                     L.ptr(kept), None, None))
    assert toks.tolist() == L.op_sample(lg, 0.7, 40, 0.9, R.SEED, R.POS0, R.N_DRAWS)[0].tolist()


@pytest.mark.parametrize("V", (300, 128256))
def test_op_logprob(V):
    lg = R.peaked_logits(V)
    toks, _, _, lp = L.op_sample_ext(lg, 1.5, 0, 1.0, R.SEED, R.POS0, R.N_DRAWS, window=X.draw_window(V), **X.CTL_ON)
    assert len(set(toks.tolist())) > 1
    for d in range(R.N_DRAWS):  # over the raw logits, whatever the controls
        want = X.logprob64(lg, int(toks[d]))
        err = abs(float(lp[d]) - want)
        assert err <= X.logprob_bound(want), (d, int(toks[d]), float(lp[d]), want, err)


# ---- the loop --------------------------------------------------------------------------------------
def hydrated(name, context=0, graphs=True):
    gm = Model.from_xalm(XalmFile(fixture_path(name + ".xalm")), context=context)
    gm.set_graphs(graphs)
    st = InferenceState(gm.config)
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    return gm, st


def run(name, n_steps, t, k=0, p=1.0, seed=0, context=0, graphs=True, history=PROMPT, pos=N, **kw):
    gm, _ = hydrated(name, context, graphs)
    out = gm.decode_sample_ext(pos, n_steps, t, k, p, seed, history=history, **kw)
    gm.close()
    return out


def replay(name, context, tokens):
    """The raw logits each token of `tokens` was drawn from: a teacher-forced xh_forward replay of
    prompt + tokens; the last entry is what the loop leaves behind."""
    gm, st = hydrated(name, context)
    out = [st.logits().copy()]
    for i, tok in enumerate(tokens):
        gm.forward(st, tok, N + i, L.OUTPUT_LOGITS)
        out.append(st.logits().copy())
    gm.close()
    return out


def replay_check(name, context, tokens, t, k, p, seed, ctl, lps=None):
    """Every token is accepted by the reference on the replayed step's l' at its counter; at
    temperature 0 it is the argmax of l' unless the top-two gap of l' is below the logit parity
    bound (undecided).  With lps: each is the float64 log-probability of its token."""
    logits = replay(name, context, tokens)
    hist = list(PROMPT)
    undecided = 0
    for i, tok in enumerate(tokens):
        raw = logits[i]
        adj = X.adjust(raw, hist, **ctl)
        if t == 0.0:
            top2 = np.sort(adj)[-2:]
            if top2[1] - top2[0] < X.parity_bound(raw):
                undecided += 1
            else:
                assert tok == int(np.argmax(np.where(adj > R.FLT_MIN, adj, -np.inf))), (i, tok)
        else:
            an = X.ExtAnalysis(adj, t, k, p, ctl.get("min_p", 0.0))
            if an.decided:
                assert tok in an.accepted(seed, N + i), (i, tok)
            else:
                undecided += 1
        if lps is not None:
            want = X.logprob64(raw, tok)
            assert abs(float(lps[i]) - want) <= X.logprob_bound(want), (i, tok, float(lps[i]), want)
        hist.append(tok)
    assert undecided <= R.SKIP_CAP * len(tokens)
    return logits


@pytest.mark.parametrize("name", FIXTURES)
def test_identity_with_decode_sample(name):
    gm, _ = hydrated(name)
    want = gm.decode_sample(N, 24, 0.9, 40, 0.95, 7)
    gm.close()
    assert len(want) == 24
    assert run(name, 24, 0.9, 40, 0.95, 7, history=()) == want
    assert run(name, 24, 0.9, 40, 0.95, 7) == want                # a history, no window
    assert run(name, 24, 0.9, 40, 0.95, 7, last_n=4) == want      # a window, every penalty off
    gm, _ = hydrated(name)
    g = gm.decode_greedy(N, 24)
    gm.close()
    assert run(name, 24, 0.0) == g


@pytest.mark.parametrize("name", FIXTURES)
def test_loop_deterministic_and_graph_independent(name):
    runs = [run(name, 30, 1.2, 40, 0.95, 11, graphs=g, logprobs=True, **LOOP_CTL) for g in (True, True, False)]
    assert len(runs[0][0]) == 30
    assert runs[0][0] == runs[1][0] == runs[2][0]
    assert bits(runs[0][1]).tolist() == bits(runs[1][1]).tolist() == bits(runs[2][1]).tolist()
    assert run(name, 30, 1.2, 40, 0.95, 12, **LOOP_CTL) != runs[0][0]


@pytest.mark.parametrize("name", FIXTURES)
def test_one_call_equals_two(name):
    whole = run(name, 8, 1.2, 50, 1.0, 21, **LOOP_CTL)
    gm, _ = hydrated(name)
    a = gm.decode_sample_ext(N, 3, 1.2, 50, 1.0, 21, history=PROMPT, **LOOP_CTL)
    b = gm.decode_sample_ext(N + 3, 5, 1.2, 50, 1.0, 21, history=PROMPT + a, **LOOP_CTL)
    gm.close()
    assert a + b == whole


@pytest.mark.parametrize("name", FIXTURES)
def test_stop_tokens(name):
    toks = run(name, 10, 1.5, 0, 1.0, 4, **LOOP_CTL)
    stop = toks[3]
    j = toks.index(stop)
    assert run(name, 10, 1.5, 0, 1.0, 4, stop=(stop, -1), **LOOP_CTL) == toks[: j + 1]


@pytest.mark.parametrize("context", (0, 16))
@pytest.mark.parametrize("name", FIXTURES)
def test_sampled_loop_against_replay(name, context):
    """30 steps (across the ring wrap with context 16): tokens, log-probabilities, and the raw logits
    the loop leaves behind."""
    t, k, p, seed = 0.9, 40, 0.95, 5
    ctl = dict(LOOP_CTL, min_p=0.02, logit_bias=[(PROMPT[1], 5.0), (7, float("-inf"))])
    gm, st = hydrated(name, context)
    toks, lps = gm.decode_sample_ext(N, 30, t, k, p, seed, history=PROMPT, logprobs=True, **ctl)
    gm.get_logits(st)
    left = st.logits().copy()
    gm.close()
    assert len(toks) == 30 and 7 not in toks
    logits = replay_check(name, context, toks, t, k, p, seed, ctl, lps)
    # get_logits is the raw lm_head output: the +5 bias of a token was not applied in place
    bound = X.parity_bound(logits[-1])
    assert float(np.abs(left - logits[-1]).max()) <= bound
    assert abs(float(left[PROMPT[1]]) - float(logits[-1][PROMPT[1]])) <= bound < 5.0 - bound


@pytest.mark.parametrize("context", (0, 16))
@pytest.mark.parametrize("name", FIXTURES)
def test_greedy_loop_with_penalties_against_replay(name, context):
    toks = run(name, 30, 0.0, context=context, **LOOP_CTL)
    assert len(toks) == 30
    replay_check(name, context, toks, 0.0, 0, 1.0, 0, LOOP_CTL)


@pytest.mark.parametrize("name", FIXTURES)
def test_logprob_matches_token_probs(name):
    gm, _ = hydrated(name)
    toks, lps = gm.decode_sample_ext(N, 12, 1.0, 0, 1.0, 9, history=PROMPT, logprobs=True, **LOOP_CTL)
    gm.reset()
    gm.set_option(L.OPT_PREFILL, 0)  # one forward per token: the logits of the decode step, bit for bit
    probs = gm.token_probs(PROMPT + toks)[N - 1:]
    gm.close()
    for i in range(12):
        want = float(np.log(np.float64(probs[i])))
        assert abs(float(lps[i]) - want) <= X.logprob_bound(want), (i, float(lps[i]), want)


@pytest.mark.parametrize("name", FIXTURES)
def test_greedy_after_ext_is_unaffected(name):
    gm, st = hydrated(name)
    toks = gm.decode_sample_ext(N, 5, 1.5, 0, 1.0, 3, history=PROMPT, **LOOP_CTL)
    cont = gm.decode_greedy(N + 5, 6)
    gm.reset()
    for pos, tok in enumerate(PROMPT + toks):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    assert gm.decode_greedy(N + 5, 6) == cont
    # and the sampled head after an extended call
    gm.reset()
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    want = gm.decode_sample(N, 6, 1.1, 0, 1.0, 2)
    gm.reset()
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    assert gm.decode_sample_ext(N, 5, 1.5, 0, 1.0, 3, history=PROMPT, **LOOP_CTL) == toks
    gm.reset()
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    assert gm.decode_sample(N, 6, 1.1, 0, 1.0, 2) == want
    gm.close()


def test_time_kernel_runs_the_extended_head():
    gm, _ = hydrated(FIXTURES[0])
    gm.decode_sample_ext(N, 1, 0.8, 40, 0.95, 1, history=PROMPT, **LOOP_CTL)
    assert gm.time_kernel(7, 4) > 0.0
    gm.close()


# ---- the CLI ---------------------------------------------------------------------------------------
def cli_ids(*args):
    path = fixture_path("tiny_mistral_f16.xalm")
    r = subprocess.run([CLI, path, "-n", "32", "-i", "the answer is", *args], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    out = r.stdout.decode("utf-8", errors="replace")
    return [int(v) for v in re.search(r"tokens: \[([0-9,]*)\]", out).group(1).split(",")]


def test_cli_penalties():
    base = cli_ids("-t", "0", "-g", "1")
    a = cli_ids("-t", "0", "-r", "1.3", "-w", "64", "-g", "1")
    assert cli_ids("-t", "0", "-r", "1.3", "-w", "64", "-g", "1") == a
    n_prompt = len(cli_ids("-n", "1", "-g", "1")) - 1
    assert a[:n_prompt] == base[:n_prompt] and len(a) > n_prompt  # a stop token may end either early
    gen = base[n_prompt:]
    assert len(set(gen)) < len(gen)  # the greedy continuation repeats within 32 tokens
    assert a != base
    # the host route (Sampler over xh_adjust_logits): both routes run the same step kernels on the
    # same prompt, so the logits agree bit for bit, l' does too, and no step is undecided
    assert cli_ids("-t", "0", "-r", "1.3", "-w", "64", "-g", "0") == a
