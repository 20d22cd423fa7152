"""Regex-constrained decoding on the device: xh_op_sample_dfa against the numpy reference
(tests/constraint_ref.py) and xh_decode_sample_dfa's loop against a teacher-forced replay on the tiny
f16 fixture."""
import ctypes
import re

import numpy as np
import pytest

import constraint_ref as C
import sample_ext_ref as X
import sample_ref as R
from conftest import fixture_path
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

FIXTURE = "tiny_mistral_f16"
PROMPT = [1, 84, 262, 259, 90]
N = len(PROMPT)
STEPS = 24
EOS = 2
# six two-letter words of the fixture's vocabulary, then a full stop or a question mark: with the end
# token at least 8 tokens (the 7 + 17 split is a real one) and at most 6 * 2 + 5 + 1 + 1 = 19 (every
# run ends on the end token within the 24 steps)
PATTERN = r"(of|to)( (of|to)){5}[.?]"
LOOP_CTL = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2, last_n=4, min_p=0.02)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the op ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.DFAS)
@pytest.mark.parametrize("V", C.VOCABS)
def test_op_matches_reference(V, name):
    nxt, acc = C.dfa(name)
    d = L.ByteDfa(nxt, acc)
    blob, offsets = L.pieces_blob(list(C.pieces(V)))
    lg = C.logits(V)
    for state, stop in C.STATES[name]:
        for draw in C.DRAWS:
            t, k, p, mp, on = draw
            ref = C.step(V, name, state, stop, draw)
            toks, kept, masked, states, lps = L.op_sample_dfa(lg, t, k, p, R.SEED, R.POS0, R.N_DRAWS, d, blob, offsets, state,
                                                            stop, window=C.window(V) if on else (), min_p=mp,
                                                            **C.controls(on))
            case = (name, state, stop, draw)
            bad = np.flatnonzero(bits(masked) != bits(ref.masked))
            assert bad.size == 0, (case, bad[:8], masked[bad[:8]], ref.masked[bad[:8]])
            assert (kept == ref.n_kept).all(), (case, kept[:4], ref.n_kept)
            skipped = 0
            for i in range(R.N_DRAWS):
                ok = ref.accepted(R.SEED, R.POS0 + i)
                if len(ok) != 1:   # within rounding of a boundary between two tokens
                    skipped += 1
                    assert int(toks[i]) in ok, (case, i)
                else:
                    assert int(toks[i]) == next(iter(ok)), (case, i, int(toks[i]), ok)
                assert int(states[i]) == ref.next_state(int(toks[i])), (case, i, int(toks[i]), int(states[i]))
            assert skipped <= C.SKIP_CAP * R.N_DRAWS, (case, skipped)
            for tok in set(toks.tolist()):   # over the raw logits, whatever the mask and the controls
                want = X.logprob64(lg, tok)
                got = lps[toks == tok]
                assert (np.abs(got.astype(np.float64) - want) <= X.logprob_bound(want)).all(), (case, tok, got[:2], want)
            if ref.stuck:
                assert set(toks.tolist()) == {C.stuck_token(stop)} and set(states.tolist()) == {C.DEAD}
            elif not ref.greedy:
                assert ref.allowed[toks].all(), case


def test_constrained_greedy_is_the_allowed_maximum():
    """Every allowed logit negative and token 0 forbidden: sample_argmax's rule would give token 0."""
    V = 4097
    nxt, acc = C.dfa("dfa3")
    d = L.ByteDfa(nxt, acc)
    blob, offsets = L.pieces_blob(list(C.pieces(V)))
    lg = (-np.abs(C.logits(V)) - 1.0).astype(np.float32)
    ref = C.Step(lg, nxt, acc, C.pieces(V), 0, C.NO_STOP, 0.0, 0, 1.0, 0.0)
    assert not ref.allowed[0] and ref.allowed.sum() >= 2
    assert L.op_sample_ext(lg, 0.0, 0, 1.0, 1, 0, 1)[0].tolist() == [0]   # the unconstrained greedy quirk
    toks, kept, masked, states, _ = L.op_sample_dfa(lg, 0.0, 0, 1.0, 1, 0, 4, d, blob, offsets, 0)
    ids = np.flatnonzero(ref.allowed)
    want = int(ids[np.argmax(lg[ids])])
    assert want == ref.token != 0
    assert toks.tolist() == [want] * 4 and kept.tolist() == [1] * 4
    assert states.tolist() == [int(ref.succ[want])] * 4
    assert (bits(masked) == bits(ref.masked)).all()


# ---- the loop --------------------------------------------------------------------------------------
def fixture_pieces():
    return L.token_pieces(XalmFile(fixture_path(FIXTURE + ".xalm")).tokens())


def hydrated(graphs=True, constraint=True):
    gm = Model.from_xalm(XalmFile(fixture_path(FIXTURE + ".xalm")))
    gm.set_graphs(graphs)
    dfa = L.regex_compile(PATTERN)
    if constraint:
        gm.set_constraint_vocab(fixture_pieces())
        gm.set_constraint(dfa)
    st = InferenceState(gm.config)
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    return gm, st, dfa


def test_pattern_fits_the_fixture():
    dfa = L.regex_compile(PATTERN)
    pieces = fixture_pieces()
    allowed, _ = C.mask(dfa.next, dfa.accept, pieces, dfa.start, (EOS, -1))
    assert allowed.sum() >= 2
    # an accepting state is reachable within the step budget: the shortest text is seven pieces, and
    # the longest (one byte per token) ends within it too
    s = dfa.start
    text = (b"of",) + (b" to",) * 5 + (b".",)
    for piece in text:
        assert piece in pieces
        s = C.walk(dfa.next, s, piece)
    assert s != C.DEAD and dfa.accept[s] and 7 < len(text) + 1 and 6 * 2 + 5 + 1 + 1 <= STEPS
    assert all(bytes([b]) in pieces for b in b"of to.?")


def replay_check(tokens, states, lps, state_in, t, k, p, seed, ctl, dfa):
    """Teacher-forced: per step xh_forward, then the reference on exactly the logits it returned."""
    gm, st, _ = hydrated(constraint=False)
    pieces = fixture_pieces()
    hist = list(PROMPT)
    state = state_in
    open_draws = 0
    for i, tok in enumerate(tokens):
        raw = st.logits().copy()
        adj = X.adjust(raw, hist, **ctl)
        ref = C.Step(adj, dfa.next, dfa.accept, pieces, state, (EOS, -1), t, k, p, ctl.get("min_p", 0.0))
        assert ref.decided and not ref.stuck, i
        ok = ref.accepted(seed, N + i)
        open_draws += len(ok) != 1
        assert tok in ok and (len(ok) != 1 or tok == next(iter(ok))), (i, tok, ok)
        assert ref.allowed[tok]
        state = ref.next_state(tok)
        assert states[i] == state, (i, states[i], state)
        want = X.logprob64(raw, tok)
        assert abs(float(lps[i]) - want) <= X.logprob_bound(want), (i, tok, float(lps[i]), want)
        hist.append(tok)
        if i + 1 < len(tokens):
            gm.forward(st, tok, N + i, L.OUTPUT_LOGITS)
    gm.close()
    assert open_draws <= C.SKIP_CAP * len(tokens)


def run(graphs, t, k, p, seed, split=None):
    """(tokens, per-step states, logprobs): one call, or `split` steps and then the rest with the
    state and the history carried; the states come from calls of one step each on a second context."""
    gm, _, dfa = hydrated(graphs)
    toks, lps, state = gm.decode_sample_dfa(N, split or STEPS, t, dfa.start, k, p, seed, history=PROMPT, stop=(EOS, -1),
                                            **LOOP_CTL)
    if split and len(toks) == split and toks[-1] != EOS:
        b, lb, state = gm.decode_sample_dfa(N + split, STEPS - split, t, state, k, p, seed, history=PROMPT + toks,
                                            stop=(EOS, -1), **LOOP_CTL)
        toks, lps = toks + b, np.concatenate([lps, lb])
    gm.close()
    return toks, lps, state, dfa


@pytest.mark.parametrize("t", (0.0, 1.1))
def test_loop_against_replay(t):
    k, p, seed = 40, 0.95, 5
    toks, lps, state, dfa = run(True, t, k, p, seed)
    assert 8 <= len(toks) <= 19
    # step by step on a second context: the state after every token
    gm, _, _ = hydrated()
    states, s = [], dfa.start
    for i in range(len(toks)):
        one, _, s = gm.decode_sample_dfa(N + i, 1, t, s, k, p, seed, history=PROMPT + toks[:i], stop=(EOS, -1), **LOOP_CTL)
        assert one == [toks[i]], (i, one, toks[i])
        states.append(s)
    gm.close()
    assert states[-1] == state
    replay_check(toks, states, lps, dfa.start, t, k, p, seed, LOOP_CTL, dfa)
    # graphs off, and split 7 + 17 with state_out carried: the same tokens, states and logprob bits
    for graphs, split in ((False, None), (True, 7), (False, 7)):
        t2, l2, s2, _ = run(graphs, t, k, p, seed, split)
        assert t2 == toks and s2 == state and bits(l2).tolist() == bits(lps).tolist(), (graphs, split)
    # the run ends on the end token (the longest text fits the budget: test_pattern_fits_the_fixture)
    # and its text matches the pattern
    pieces = fixture_pieces()
    assert toks[-1] == EOS and EOS not in toks[:-1]
    text = b"".join(pieces[tok] for tok in toks[:-1])
    assert re.fullmatch(PATTERN.encode(), text), text
    assert dfa.accept[state]


def test_other_loops_do_not_read_the_constraint():
    gm, _, _ = hydrated(constraint=False)
    ext = gm.decode_sample_ext(N, 12, 0.9, 40, 0.95, 7, history=PROMPT, **LOOP_CTL)
    gm.close()
    gm, _, _ = hydrated(constraint=False)
    greedy = gm.decode_greedy(N, 12)
    gm.close()
    gm, _, dfa = hydrated()
    gm.decode_sample_dfa(N, 2, 0.9, dfa.start, 40, 0.95, 7, history=PROMPT, **LOOP_CTL)  # the new graph exists too
    st = InferenceState(gm.config)
    for kind in ("ext", "greedy"):
        gm.reset()
        for pos, tok in enumerate(PROMPT):
            gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
        if kind == "ext":
            assert gm.decode_sample_ext(N, 12, 0.9, 40, 0.95, 7, history=PROMPT, **LOOP_CTL) == ext
        else:
            assert gm.decode_greedy(N, 12) == greedy
    assert set(ext) != {EOS} and not re.fullmatch(PATTERN.encode(), b"".join(fixture_pieces()[t] for t in ext))
    gm.close()


def test_stuck_state_in_the_loop():
    """A hand-made DFA that reads one `a` and then nothing: the second step is stuck and emits the end
    token; without end tokens it emits 0 from then on and the state stays XH_DFA_DEAD."""
    nxt = np.full((2, 256), C.DEAD, np.uint16)
    nxt[0, ord("a")] = 1
    dfa = L.ByteDfa(nxt, np.zeros(2, np.uint8))
    gm, _, _ = hydrated(constraint=False)
    gm.set_constraint_vocab(fixture_pieces())
    gm.set_constraint(dfa)
    a = [t for t, piece in enumerate(fixture_pieces()) if piece == b"a"]   # the letter and its byte-fallback token
    assert len(a) == 2
    toks, _, state = gm.decode_sample_dfa(N, 4, 0.8, 0, seed=3, history=PROMPT)
    assert toks[0] in a and toks[1:] == [0, 0, 0] and state == C.DEAD
    toks, _, state = gm.decode_sample_dfa(N, 4, 0.8, 0, seed=3, history=PROMPT, stop=(-1, EOS))
    assert toks[0] in a and toks[1:] == [EOS] and state == C.DEAD
    toks, _, state = gm.decode_sample_dfa(N, 2, 0.8, C.DEAD, seed=3, history=PROMPT)   # DEAD is a valid state_in
    assert toks == [0, 0] and state == C.DEAD
    assert gm.time_kernel(8, 4) > 0.0
    gm.close()


def test_invalid_arguments_with_a_context():
    gm, _, dfa = hydrated(constraint=False)
    pieces = fixture_pieces()

    def decode_rc(state=0, stop=(-1, -1)):
        s = L.XhSampling(0.8, 0, 1.0, 0)
        toks = np.zeros(4, np.int32)
        done = ctypes.c_int(0)
        return L.lib().xh_decode_sample_dfa(gm._ctx, N, 2, ctypes.byref(s), None, None, 0, state, stop[0], stop[1],
                                            L.ptr(toks), None, None, ctypes.byref(done))

    INVALID = 1
    assert decode_rc() == INVALID                       # before both uploads
    assert L.lib().xh_time_kernel(gm._ctx, 8, 2, ctypes.byref(ctypes.c_float(0))) == 3
    gm.set_constraint_vocab(pieces)
    assert decode_rc() == INVALID                       # the pieces alone
    gm.set_constraint(dfa)
    assert decode_rc() == 0
    assert gm.time_kernel(8, 2) > 0.0
    # the timing hook reads the tables through the block the decode call writes: refused (XH_E_STATE)
    # after either upload until a decode call has rewritten it
    us = ctypes.c_float(0)
    gm.set_constraint(dfa)
    assert L.lib().xh_time_kernel(gm._ctx, 8, 2, ctypes.byref(us)) == 3
    assert decode_rc() == 0 and gm.time_kernel(8, 2) > 0.0
    gm.set_constraint_vocab(pieces)
    assert L.lib().xh_time_kernel(gm._ctx, 8, 2, ctypes.byref(us)) == 3
    assert decode_rc() == 0
    gm.set_constraint(None)
    assert decode_rc() == INVALID                       # cleared
    gm.set_constraint(dfa)
    assert decode_rc(state=dfa.n_states) == INVALID
    assert decode_rc(state=C.DEAD) == 0
    assert decode_rc(stop=(gm.config.vocab_size, -1)) == INVALID
    wrong = dfa.next.copy()
    wrong[dfa.start, ord("t")] = dfa.n_states           # neither a state nor XH_DFA_DEAD
    bad = L.ByteDfa(wrong, dfa.accept, dfa.start)
    for d in (bad.abi(), dfa.abi(0), L.ByteDfa(dfa.next, dfa.accept, dfa.n_states).abi(),
              L.XhByteDfa(dfa.n_states, 0, None, dfa.accept.ctypes.data)):
        assert L.lib().xh_constraint_set(gm._ctx, ctypes.byref(d)) == INVALID
    assert decode_rc() == 0                             # a refused DFA leaves the old one in place
    blob, offsets = L.pieces_blob(pieces)
    off2 = offsets.copy()
    off2[0] = 1
    assert L.lib().xh_constraint_set_vocab(gm._ctx, L.ptr(blob), L.ptr(off2)) == INVALID
    assert L.lib().xh_constraint_set_vocab(gm._ctx, None, L.ptr(offsets)) == INVALID
    gm.close()
