"""The top-N log-probabilities on the device: xh_op_top_logprobs over the shared case list, the four
decode loops under xh_set_top_logprobs against the reference applied to the very logits bits each
step chose from, xh_score against its own echoed logits, xh_perplexity and per-token forwards, and
the CLI's -L.  Every comparison is on identical bits, so nothing is skipped as undecided."""
import os
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import top_logprobs_ref as T
from conftest import ROOT, fixture_path
from sample_ext_ref import logprob_bound, parity_bound
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "xalm_amd", "bin", "xalm")
FIXTURES = ["tiny_mistral_f16", "small_llama_f16"]
PROMPT = [1, 84, 262, 259, 90]
N = len(PROMPT)
STEPS = 12
N_TOP = 5
LOOPS = ("greedy", "sample", "ext", "dfa")
CTL = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2, last_n=4, min_p=0.02)
FLT_MIN = float(np.finfo(np.float32).tiny)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the op ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", T.N_ROWS)
@pytest.mark.parametrize("V", T.VOCABS)
def test_op_matches_reference(V, n_rows):
    for name, (lg, tg) in T.cases(V, n_rows).items():
        for n_top in T.N_TOPS:
            got = L.op_top_logprobs(lg, n_top, tg)
            T.check_rows(lg, n_top, tg, got, (name, V, n_top))
            if n_top == 5:
                again = L.op_top_logprobs(lg, n_top, tg)
                for a, b in zip(got, again):
                    assert a.tobytes() == b.tobytes(), (name, V)
                ids, lps = L.op_top_logprobs(lg, n_top)      # no targets: the same lists
                assert ids.tobytes() == got[0].tobytes() and lps.tobytes() == got[1].tobytes(), (name, V)


@pytest.mark.parametrize("V", T.VOCABS)
def test_op_70_rows(V):
    """More rows than one wave of workgroups, each row its own data: a row-stride error shows;
    V = 128256 and 1025 are no multiples of 1024."""
    rows = 70
    rng = np.random.default_rng(99 + V)
    lg = (rng.standard_normal((rows, V)) * 3.0).astype(np.float32)
    lg[1::3] = np.round(lg[1::3])            # every third row: tie blocks
    tg = rng.integers(0, V, rows).astype(np.int32)
    got = L.op_top_logprobs(lg, 5, tg)
    T.check_rows(lg, 5, tg, got, ("70_rows", V))
    again = L.op_top_logprobs(lg, 5, tg)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()


# ---- the decode loops ------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def pieces(V):
    return tuple(b"a" for _ in range(V))    # with the DFA of a*: every token allowed in every state


def hydrated(name, n_top, graphs=True):
    gm = Model.from_xalm(XalmFile(fixture_path(name + ".xalm")))
    gm.set_graphs(graphs)
    gm.set_constraint_vocab(list(pieces(gm.config.vocab_size)))
    dfa = L.regex_compile("a*")
    gm.set_constraint(dfa)
    gm.dfa_start = dfa.start
    gm.set_top_logprobs(n_top)
    st = InferenceState(gm.config)
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    return gm, st


def step_call(gm, loop, pos, n, done, state):
    """One call of `loop` for n steps at pos after the tokens `done`; returns (tokens, logprobs or
    None, DFA state)."""
    if loop == "greedy":
        return gm.decode_greedy(pos, n), None, state
    if loop == "sample":
        return gm.decode_sample(pos, n, 0.9, 40, 0.95, 11), None, state
    if loop == "ext":
        toks, lps = gm.decode_sample_ext(pos, n, 0.9, 40, 0.95, 11, history=PROMPT + done, logprobs=True, **CTL)
        return toks, lps, state
    toks, lps, state = gm.decode_sample_dfa(pos, n, 0.9, state, 40, 0.95, 11, history=PROMPT + done, **CTL)
    return toks, lps, state


def run_split(name, loop, splits, n_top=N_TOP, graphs=True):
    """The STEPS steps as calls of the given lengths: (tokens, logprobs, ids, lps, ranks, the logits
    before each call)."""
    gm, st = hydrated(name, n_top, graphs)
    toks, lps_out, ids, lps, ranks, logits = [], [], [], [], [], []
    state = gm.dfa_start
    for n in splits:
        gm.get_logits(st)
        logits.append(st.logits().copy())
        t, lp, state = step_call(gm, loop, N + len(toks), n, toks, state)
        assert len(t) == n
        if n_top:
            i, l, r = gm.top_logprobs(n)
            ids.append(i.copy()); lps.append(l.copy()); ranks.append(r.copy())
        toks += t
        if lp is not None:
            lps_out += list(lp)
    gm.close()
    cat = (lambda a: np.concatenate(a)) if n_top else (lambda a: None)
    return toks, lps_out, cat(ids), cat(lps), cat(ranks), logits


@lru_cache(maxsize=None)
def one_step_rows(name, loop):
    return run_split(name, loop, (1,) * STEPS)


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("name", FIXTURES)
def test_loop_rows_match_reference_on_the_steps_logits(name, loop):
    toks, lp_out, ids, lps, ranks, logits = one_step_rows(name, loop)
    for i in range(STEPS):
        T.check_rows(logits[i], N_TOP, [toks[i]],
                     (ids[i:i + 1], lps[i:i + 1], _target_lps(logits[i], toks[i]), ranks[i:i + 1]), (name, loop, i))
    if lp_out:
        # lps[rank] is the emitted token's own entry where it made the list; the two sums are
        # evaluated separately: twice the bound
        seen = 0
        for i in range(STEPS):
            if ranks[i] < N_TOP:
                assert ids[i][ranks[i]] == toks[i]
                assert abs(float(lps[i][ranks[i]]) - float(lp_out[i])) <= 2 * logprob_bound(float(lp_out[i])), (name, loop, i)
                seen += 1
        assert seen > 0


def _target_lps(logits, tok):
    # the loops report no target log-probability of their own (logprobs_out is the heads'): feed
    # check_rows the reference value so that only ids, lps and ranks are compared
    return np.array([T.logprobs64(logits)[tok]])


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("name", FIXTURES)
def test_loop_rows_are_split_and_graph_independent(name, loop):
    toks, _, ids, lps, ranks, _ = one_step_rows(name, loop)
    for splits, graphs in (((STEPS,), True), ((5, 7), True), ((STEPS,), False)):
        t, _, i, l, r, _ = run_split(name, loop, splits, graphs=graphs)
        assert t == toks, (splits, graphs)
        assert i.tobytes() == ids.tobytes() and l.tobytes() == lps.tobytes() and r.tobytes() == ranks.tobytes(), (splits, graphs)
    # the draw is untouched: the same loop with n_top = 0 emits the same tokens
    t0, *_ = run_split(name, loop, (STEPS,), n_top=0)
    assert t0 == toks


def test_width_changes_without_a_new_capture_and_state_errors():
    gm, st = hydrated(FIXTURES[0], 0)
    rc = L.lib().xh_get_top_logprobs(gm._ctx, 1, None, None, None)
    assert rc == 3                                                   # XH_E_STATE: n_top is 0
    gm.set_top_logprobs(3)
    assert L.lib().xh_get_top_logprobs(gm._ctx, 1, None, None, None) == 3   # no call since
    gm.get_logits(st)
    lg = st.logits().copy()
    toks = gm.decode_greedy(N, 2)
    ids3, lps3, r3 = gm.top_logprobs(2)
    assert ids3.shape == (2, 3) and r3.tolist() == [0, 0] and ids3[:, 0].tolist() == toks
    assert ids3[0].tolist() == T.top(lg, 3)[0].tolist()
    assert L.lib().xh_get_top_logprobs(gm._ctx, 3, None, None, None) == 1   # XH_E_INVALID: 2 steps ran
    gm.set_top_logprobs(32)                                          # a wider list, the same graph
    gm.get_logits(st)
    lg = st.logits().copy()
    gm.decode_greedy(N + 2, 1)
    ids32, lps32, _ = gm.top_logprobs(1)
    T.check_rows(lg, 32, None, (ids32, lps32), "width_32")
    for bad in (-1, 33):
        assert L.lib().xh_set_top_logprobs(gm._ctx, bad) == 1
    assert gm.time_kernel(9, 4) > 0.0 and gm.kernel_bytes(9, 0) > 0
    gm.set_top_logprobs(0)
    with pytest.raises(L.XhError):
        gm.time_kernel(9, 4)                                         # XH_E_STATE: nothing to time at width 0
    gm.close()


# ---- xh_score --------------------------------------------------------------------------------------
SCORE_TOKENS = [1] + [int(t) for t in np.random.default_rng(5).integers(3, 300, 39)]
assert len(SCORE_TOKENS) == 40


@pytest.mark.parametrize("prefill", (1, 0))
@pytest.mark.parametrize("context", (0, 16))
@pytest.mark.parametrize("name", FIXTURES)
def test_score(name, context, prefill):
    """40 tokens at pos0 = 0; context 16 crosses the ring wrap (ring passes on small_llama's
    head_dim 128, the token loop on tiny_mistral's 16)."""
    gm = Model.from_xalm(XalmFile(fixture_path(name + ".xalm")), context=context)
    gm.set_option(L.OPT_PREFILL, prefill)
    toks = SCORE_TOKENS
    m = len(toks) - 1
    out = gm.score(toks, 0, N_TOP, echo_logits=True)
    lg = out["logits"]
    tg = np.array(toks[1:], dtype=np.int32)
    T.check_rows(lg, N_TOP, tg, (out["top_ids"], out["top_logprobs"], out["logprobs"], out["ranks"]), (name, context, prefill))
    # n_top = 0 and no echo: the same figures
    lean = gm.score(toks, 0)
    assert lean["logprobs"].tobytes() == out["logprobs"].tobytes() and lean["ranks"].tobytes() == out["ranks"].tobytes()
    # xh_perplexity's probabilities: its maximum starts at FLT_MIN, the same wherever the row's exceeds that
    assert (lg.max(axis=1) > FLT_MIN).all()
    probs = gm.token_probs(toks, 0)
    for i in range(m):
        lp = float(out["logprobs"][i])
        rel = 2e-5 + 2.0 ** -21 * max(1.0, abs(lp))
        # probs is an f32 quotient: below the normal range (FLT_MIN) it is a denormal or flushed to
        # 0, where no relative bound can hold (the underflow xh_score exists to avoid), so the
        # bound carries FLT_MIN as its absolute floor
        assert abs(np.exp(lp) - float(probs[i])) <= rel * float(probs[i]) + FLT_MIN, (i, lp, float(probs[i]))
    # the echoed logits against per-token forwards at the same positions
    gm.reset()
    st = InferenceState(gm.config)
    for i in range(m):
        gm.forward(st, toks[i], i, L.OUTPUT_LOGITS)
        ref = st.logits()
        assert float(np.abs(lg[i] - ref).max()) <= parity_bound(ref), (name, context, prefill, i)
    gm.close()


def test_score_invalid_arguments():
    gm = Model.from_xalm(XalmFile(fixture_path(FIXTURES[0] + ".xalm")))
    lib = L.lib()
    toks = np.array(SCORE_TOKENS[:4], dtype=np.int32)
    lp = np.zeros(3, dtype=np.float32)
    call = lambda t, n, pos0, n_top: lib.xh_score(gm._ctx, L.ptr(t) if t is not None else None, n, pos0, n_top,  # noqa: E731
                                                  L.ptr(lp), None, None, None, None)
    assert call(toks, 4, 0, 0) == 0
    assert call(toks, 1, 0, 0) == 1 and call(None, 4, 0, 0) == 1 and call(toks, 4, -1, 0) == 1
    assert call(toks, 4, 0, -1) == 1 and call(toks, 4, 0, 33) == 1
    bad = toks.copy()
    bad[2] = gm.config.vocab_size
    assert call(bad, 4, 0, 0) == 1
    gm.close()


# ---- the CLI ---------------------------------------------------------------------------------------
def cli(*args):
    path = fixture_path("tiny_mistral_f16.xalm")
    r = subprocess.run([CLI, path, "-n", "8", "-i", "the answer is", *args], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    out = r.stdout.decode("utf-8", errors="replace")
    return out, [int(v) for v in re.search(r"tokens: \[([0-9,]*)\]", out).group(1).split(",")]


@pytest.mark.parametrize("g", ("1", "0"))
def test_cli_top_logprobs(g):
    _, base = cli("-g", g)
    out, ids = cli("-g", g, "-L", "3")
    assert ids == base
    rows = re.findall(r"^top: token (\d+) rank (\d+) \|((?: \d+:-?[0-9.einf+-]+){3})$", out, re.M)
    n_prompt = len(cli("-g", g, "-n", "1")[1]) - 1
    assert len(rows) == len(ids) - n_prompt > 0
    for (tok, rank, alts), want in zip(rows, ids[n_prompt:]):
        assert int(tok) == want and int(rank) == 0             # greedy: the token is the first alternative
        first = alts.split()[0]
        assert int(first.split(":")[0]) == want
