"""Regex-constrained decoding without a device: xh_regex_compile against Python's re,
xh_constraint_mask against the numpy reference (tests/constraint_ref.py), the argument checks that
run before the device is touched, and the reference's own decidedness on the GPU test's cases."""
import ctypes
import itertools
import re

import numpy as np
import pytest

import constraint_ref as C
import sample_ref as R
from xalm_amd import _lib as L

ALPHABET = 'ab0 -"'
PATTERNS = [
    r"ab",                     # literals
    r"a|b0|",                  # alternation, an empty branch
    r"(a|b)*0",                # alternation under a star
    r"(ab|a)*",
    r"a{2,3}b?",               # {m,n} and ?
    r"a{2}-{1,}",              # {m} and {m,}
    r"[^ab]+",                 # a negated class, +
    r"\d+(\.\d+)?",            # the issue's number
    r'"[a-b0 ]*"',             # a range in a class
    r".?b",                    # any byte
    r"[a-b]{0,2}0+",
    r'\x61\-\"\\?',            # \xHH and escaped punctuation
    r"\s\w*",                  # \s \w
    r"(a|)(b|0){2}( |-)",
    r"[]a][\d -]*",            # a leading ] and a class escape
]
WORDS = ["".join(t) for n in range(6) for t in itertools.product(ALPHABET, repeat=n)]


def matches(d, data):
    s = d.start
    for b in data:
        s = int(d.next[s, b])
        if s == L.DFA_DEAD:
            return False
    return bool(d.accept[s])


def compile_rc(pattern, cap=0):
    n, start = ctypes.c_int(-1), ctypes.c_int(-1)
    nxt = np.zeros((max(cap, 1), 256), np.uint16)
    acc = np.zeros(max(cap, 1), np.uint8)
    rc = L.lib().xh_regex_compile(pattern.encode(), L.ptr(nxt), L.ptr(acc), cap, ctypes.byref(n), ctypes.byref(start))
    return rc, n.value


@pytest.mark.parametrize("pattern", PATTERNS)
def test_regex_matches_python_re(pattern):
    d = L.regex_compile(pattern)
    rx = re.compile(pattern.encode())
    bad = [w for w in WORDS if matches(d, w.encode()) != bool(rx.fullmatch(w.encode()))]
    assert not bad, (pattern, bad[:8])
    assert any(rx.fullmatch(w.encode()) for w in WORDS), pattern  # the comparison is not vacuous


@pytest.mark.parametrize("pattern", PATTERNS + [r"(a{200}){200}", r"(ab|cd|e[f-h]+){3,}x"])
def test_regex_dfa_is_trimmed(pattern):
    d = L.regex_compile(pattern)
    n = d.n_states
    assert 0 <= d.start < n and d.accept.any()
    table = d.next.astype(np.int64)
    assert ((table < n) | (table == L.DFA_DEAD)).all()
    # graph search over the distinct edges: every state reaches an accepting state (backward from
    # them), and the start reaches every state (subset construction builds no other)
    src, dst = np.nonzero(table != L.DFA_DEAD)
    dst = table[src, dst]
    edges = np.unique(np.stack([src, dst], axis=1), axis=0)
    assert reach(n, edges[:, 1], edges[:, 0], np.flatnonzero(d.accept)).all()
    assert reach(n, edges[:, 0], edges[:, 1], [d.start]).all()


def reach(n, src, dst, roots):
    """bool [n]: the states a breadth-first search along src -> dst reaches from `roots`."""
    order = np.argsort(src, kind="stable")
    src, dst = src[order], dst[order]
    first = np.searchsorted(src, np.arange(n + 1))
    seen = np.zeros(n, bool)
    seen[roots] = True
    frontier = list(roots)
    while frontier:
        out = np.concatenate([dst[first[s]:first[s + 1]] for s in frontier])
        out = np.unique(out[~seen[out]])
        seen[out] = True
        frontier = out.tolist()
    return seen


def test_regex_number_with_a_fraction():
    """The issue's alphabet has no full stop: the optional fraction of the number pattern, here."""
    pattern = r"\d+(\.\d+)?"
    d = L.regex_compile(pattern)
    rx = re.compile(pattern.encode())
    words = ["".join(t) for n in range(6) for t in itertools.product("07.a", repeat=n)]
    assert [w for w in words if matches(d, w.encode()) != bool(rx.fullmatch(w.encode()))] == []
    assert matches(d, b"12.5") and not matches(d, b"12.") and not matches(d, b".5")


def test_regex_nesting_is_capped():
    assert compile_rc("(" * 256 + "a" + ")" * 256, 4) == (0, 2)
    assert compile_rc("(" * 257 + "a" + ")" * 257, 4)[0] == 1
    assert compile_rc("(" * 200000 + "a" + ")" * 200000, 4)[0] == 1   # XH_E_INVALID, not a stack overflow


def test_token_pieces_byte_fallback():
    toks = [b"<unk>", b"<s>"] + [b"<0x%02X>" % i for i in range(256)] + [b"a", b" the"]
    out = L.token_pieces(toks)
    assert out[:2] == toks[:2] and out[2:258] == [bytes([i]) for i in range(256)] and out[258:] == toks[258:]
    short = toks[:100]                       # no whole run of 256: the names stay as they are
    assert L.token_pieces(short) == short


def test_regex_utf8_is_bytes():
    d = L.regex_compile("é+")   # two bytes: the + binds the second
    assert matches(d, "é".encode()) and matches(d, b"\xc3\xa9\xa9") and not matches(d, "éé".encode())
    assert matches(L.regex_compile("(é)+"), "éé".encode())
    dot = L.regex_compile(".*")
    assert dot.n_states == 1 and matches(dot, b"") and matches(dot, bytes(range(11, 256))) and not matches(dot, b"a\nb")


def test_regex_error_codes():
    XH_E_INVALID, XH_E_NOMEM = 1, 4
    for bad in ["a**", "(", "a)", "[a", "a{2", "a{3,2}", "a{257}", "*a", r"\q", "a{", "a+?", r"\x4"]:
        assert compile_rc(bad, 16)[0] == XH_E_INVALID, bad
    assert compile_rc(r"a[^\x00-\xff]", 16)[0] == XH_E_INVALID          # the empty language
    assert compile_rc(r"(a{256}){256}b", 16)[0] == XH_E_INVALID         # more than XH_DFA_MAX_STATES states
    assert compile_rc(r"\d+(\.\d+)?", 3) == (XH_E_NOMEM, 4)              # the cap is too small: the size comes back
    assert compile_rc(r"\d+(\.\d+)?", 4) == (0, 4)
    n = ctypes.c_int(0)
    assert L.lib().xh_regex_compile(None, None, None, 0, ctypes.byref(n), ctypes.byref(n)) == XH_E_INVALID


# ---- xh_constraint_mask against the reference ------------------------------------------------------
@pytest.mark.parametrize("name", C.DFAS)
def test_constraint_mask_matches_reference(name):
    V = 4097
    nxt, acc = C.dfa(name)
    d = L.ByteDfa(nxt, acc)
    pieces = C.pieces(V)
    assert pieces[4] == b"" and len(pieces[6]) == 300 and {len(p) for p in pieces} >= set(range(1, 10))
    blob, offsets = L.pieces_blob(list(pieces))
    for state, stop in C.STATES[name]:
        want_allowed, want_succ = C.mask(nxt, acc, pieces, state, stop)
        allowed, succ = L.constraint_mask(d, blob, offsets, state, stop)
        assert (allowed.astype(bool) == want_allowed).all(), (state, stop)
        assert (succ == want_succ).all(), (state, stop, np.flatnonzero(succ != want_succ)[:8])
        assert not allowed[4]                                    # the empty piece
        for t in stop:
            if t >= 0 and state != C.DEAD:
                assert bool(allowed[t]) == bool(acc[state]) and (not allowed[t] or succ[t] == state)
        # the numpy walk and the scalar one agree on a sample
        for t in list(range(12)) + [V - 1]:
            if t not in stop:
                assert int(want_succ[t]) == C.walk(nxt, state, pieces[t])
    if name == "dfa700":   # states above 255 are reached and told apart (an 8-bit state id would alias them)
        _, succ = L.constraint_mask(d, blob, offsets, 250, C.NO_STOP)
        assert succ[6] == (250 + 300) % 700 and succ[7] == 252 and succ[10] == 259
    if name == "chain":    # states above 32767 (a signed 16-bit state id would go negative)
        _, succ = L.constraint_mask(d, blob, offsets, 32767, C.NO_STOP)
        assert succ[1] == 32768 and succ[6] == 33067
        allowed, _ = L.constraint_mask(d, blob, offsets, 39990, C.NO_STOP)
        assert allowed[10] and not allowed[6]                    # 9 more fit, 300 do not


# ---- the arguments, checked before any device work -------------------------------------------------
def mask_rc(d, blob, offsets, V, state=0):
    allowed = np.zeros(max(V, 1), np.uint8)
    succ = np.zeros(max(V, 1), np.uint16)
    return L.lib().xh_constraint_mask(ctypes.byref(d) if d is not None else None, L.ptr(blob) if blob is not None else None,
                                      L.ptr(offsets) if offsets is not None else None, V, state, -1, -1,
                                      L.ptr(allowed), L.ptr(succ))


def op_rc(d, blob, offsets, V, state=0, stop=(-1, -1)):
    lg = np.zeros(max(V, 1), np.float32)
    s = L.XhSampling(0.0, 0, 1.0, 0)
    out = np.zeros(4, np.int32)
    st = np.zeros(4, np.uint32)
    return L.lib().xh_op_sample_dfa(L.ptr(lg), V, ctypes.byref(s), None, None, 0, ctypes.byref(d) if d is not None else None,
                                    L.ptr(blob) if blob is not None else None,
                                    L.ptr(offsets) if offsets is not None else None, state, stop[0], stop[1], 0, 1,
                                    L.ptr(out), L.ptr(out), None, L.ptr(st), None)


def test_invalid_arguments_without_a_device():
    XH_E_INVALID = 1
    V = 97
    nxt, acc = C.dfa("dfa3")
    good = L.ByteDfa(nxt, acc)
    blob, offsets = L.pieces_blob(list(C.pieces(V)))
    assert mask_rc(good.abi(), blob, offsets, V) == 0
    assert mask_rc(good.abi(), blob, offsets, V, C.DEAD) == 0     # the stuck state is a valid state_in
    bad_next = L.ByteDfa(np.where(nxt == 2, 3, nxt), acc)          # 3 is neither < n_states nor DEAD
    not_from_0 = offsets.copy()
    not_from_0[0] = 1
    descending = offsets.copy()
    descending[10] = descending[9] - 1
    too_big = offsets.copy()
    too_big[-1] = (16 << 20) + 1
    wide = np.zeros((1 << 17) + 2, np.uint32)
    rows = {
        "n_states 0": (good.abi(0), blob, offsets, V, 0),
        "n_states 65536": (good.abi(65536), blob, offsets, V, 0),
        "start out of range": (L.ByteDfa(nxt, acc, 3).abi(), blob, offsets, V, 0),
        "start negative": (L.ByteDfa(nxt, acc, -1).abi(), blob, offsets, V, 0),
        "state out of range": (good.abi(), blob, offsets, V, 3),
        "next entry out of range": (bad_next.abi(), blob, offsets, V, 0),
        "null next": (L.XhByteDfa(3, 0, None, acc.ctypes.data), blob, offsets, V, 0),
        "null accept": (L.XhByteDfa(3, 0, nxt.ctypes.data, None), blob, offsets, V, 0),
        "null dfa": (None, blob, offsets, V, 0),
        "null bytes": (good.abi(), None, offsets, V, 0),
        "null offsets": (good.abi(), blob, None, V, 0),
        "offsets not from 0": (good.abi(), blob, not_from_0, V, 0),
        "offsets descending": (good.abi(), blob, descending, V, 0),
        "blob over 16 MiB": (good.abi(), blob, too_big, V, 0),
        "vocab over 2^17": (good.abi(), blob, wide, (1 << 17) + 1, 0),
    }
    for why, (d, b, o, v, state) in rows.items():
        assert mask_rc(d, b, o, v, state) == XH_E_INVALID, why
        assert op_rc(d, b, o, v, state) == XH_E_INVALID, why      # the device op: refused before any device work
    assert op_rc(good.abi(), blob, offsets, V, 0, stop=(V, -1)) == XH_E_INVALID   # the stuck state would emit it


# ---- the GPU test's cases are decided by the reference alone -----------------------------------------
@pytest.mark.parametrize("V", C.VOCABS)
def test_draw_cases_are_decided(V):
    kinds = set()
    for name in C.DFAS:
        for state, stop in C.STATES[name]:
            for draw in C.DRAWS:
                st = C.step(V, name, state, stop, draw)
                assert st.decided, (name, state, stop, draw)
                kinds.add("stuck" if st.stuck else "greedy" if st.greedy else "sampled")
                if st.an is not None and st.n_kept > 0:
                    open_draws = sum(len(st.accepted(R.SEED, R.POS0 + d)) != 1 for d in range(R.N_DRAWS))
                    assert open_draws <= C.SKIP_CAP * R.N_DRAWS, (name, state, stop, draw, open_draws)
    assert kinds == {"stuck", "greedy", "sampled"}


def test_reference_greedy_rule():
    """All allowed logits negative and token 0 forbidden: the allowed maximum, not sample_argmax's 0."""
    V = 97
    nxt, acc = C.dfa("dfa3")
    lg = (-np.abs(C.logits(V)) - 1.0).astype(np.float32)
    st = C.Step(lg, nxt, acc, C.pieces(V), 0, C.NO_STOP, 0.0, 0, 1.0, 0.0)
    ids = np.flatnonzero(st.allowed)
    assert not st.allowed[0] and ids.size >= 2
    assert st.token == int(ids[np.argmax(lg[ids])]) and st.token != 0
