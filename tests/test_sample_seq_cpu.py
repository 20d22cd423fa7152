"""The sequence-aware draw without a GPU: the new symbols, parameter validation before the device is
touched, xh_seq_adjust_host and xh_xtc_host against the reference (tests/sample_seq_ref.py) on the
case lists, and the skip cap of the GPU tests' case lists on the reference alone."""
import ctypes

import numpy as np
import pytest

import sample_ext_ref as X
import sample_ref as R
import sample_seq_ref as Q
from xalm_amd import _lib as L

NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_symbols_exported():
    lib = L.lib()
    for name in ("xh_decode_sample_seq", "xh_op_sample_seq", "xh_seq_adjust_host", "xh_xtc_host"):
        assert hasattr(lib, name), name
    import xalm_amd
    assert callable(xalm_amd.op_sample_seq) and callable(xalm_amd.seq_adjust_host) and callable(xalm_amd.xtc_host)
    assert hasattr(xalm_amd.Model, "decode_sample_seq")
    assert (L.SEQ_MAX_MATCH, L.SEQ_MAX_BREAKERS) == (Q.MAX_MATCH, 1024)


# ---- invalid arguments ---------------------------------------------------------------------------
V_BAD = 64
BAD = [
    dict(dry_multiplier=-0.1), dict(dry_multiplier=INF), dict(dry_multiplier=NAN),
    dict(dry_base=0.99), dict(dry_base=INF), dict(dry_base=NAN),
    dict(dry_allowed_length=0), dict(dry_allowed_length=65), dict(dry_allowed_length=-3),
    dict(no_repeat_ngram=1), dict(no_repeat_ngram=65), dict(no_repeat_ngram=-2),
    dict(seq_last_n=-1), dict(seq_last_n=1025),
    dict(breakers=(3, 3)), dict(breakers=(-1,)), dict(breakers=(V_BAD,)),
    dict(xtc_probability=-0.1), dict(xtc_probability=1.1), dict(xtc_probability=NAN),
    dict(xtc_threshold=0.0), dict(xtc_threshold=1.5), dict(xtc_threshold=NAN),
]


def call_all(q, trunc=None, s=None, host=True, null_seq=False):
    """(xh_decode_sample_seq with a null context, xh_op_sample_seq, xh_seq_adjust_host, xh_xtc_host) return codes."""
    lib = L.lib()
    lg = np.zeros(V_BAD, np.float32)
    toks, kept = np.zeros(4, np.int32), np.zeros(4, np.int32)
    st, mus = np.zeros(4, np.uint32), np.zeros(4, np.float32)
    k8 = np.ones(V_BAD, np.uint8)
    done = ctypes.c_int(-1)
    s = s or L.XhSampling(1.0, 0, 1.0, 1)
    t = trunc or L.XhTruncCtl(1.0, 0.0, 0.0, 0.1)
    mu = 2.0 * t.mirostat_tau
    qp = None if null_seq else ctypes.byref(q)
    a = lib.xh_decode_sample_seq(None, 0, 4, ctypes.byref(s), None, ctypes.byref(t), qp, None, 0, 0, 0, mu, -1, -1, L.ptr(toks),
                                 None, None, None, ctypes.byref(done))
    assert done.value == 0
    b = lib.xh_op_sample_seq(L.ptr(lg), V_BAD, ctypes.byref(s), None, ctypes.byref(t), qp, None, 0, None, None, None, 0, mu, -1,
                             -1, 0, 4, L.ptr(toks), L.ptr(kept), L.ptr(st), L.ptr(mus), None, None, None, None, None)
    if not host:
        return a, b
    c = lib.xh_seq_adjust_host(L.ptr(lg), V_BAD, qp, None, 0, None, None, None)
    d = lib.xh_xtc_host(L.ptr(lg), V_BAD, 1.0, qp, 1, 0, L.ptr(k8), None, None)
    return a, b, c, d


@pytest.mark.parametrize("case", BAD, ids=[str(i) for i in range(len(BAD))])
def test_invalid_seq_rejected_before_the_device(case):
    q, keep = L.seq_ctl(**case)
    assert call_all(q) == (1, 1, 1, 1), case
    assert L.lib().xh_last_error(None)
    del keep


def test_invalid_composed_arguments_rejected():
    good, keep = L.seq_ctl(dry_multiplier=0.8, seq_last_n=64, xtc_probability=0.5)
    assert call_all(good, null_seq=True) == (1, 1, 1, 1)
    # n_breakers > 0 with a null array
    q = L.XhSeqCtl(0.8, 1.75, 2, 0, 64, 3, None, 0.0, 0.1)
    assert call_all(q) == (1, 1, 1, 1)
    # Mirostat excludes XTC; without XTC it is accepted as far as the arguments go (a null context: 1 either way)
    miro = L.XhTruncCtl(1.0, 0.0, 3.0, 0.1)
    assert call_all(good, trunc=miro, host=False) == (1, 1)
    assert b"xtc_probability" in L.lib().xh_last_error(None)
    # what xh_decode_sample_adapt rejects: sampling and xh_trunc_ctl
    off, keep2 = L.seq_ctl()
    assert call_all(off, s=L.XhSampling(-1.0, 0, 1.0, 1), host=False) == (1, 1)
    assert call_all(off, trunc=L.XhTruncCtl(0.0, 0.0, 0.0, 0.1), host=False) == (1, 1)
    # 1024 breakers are the most: one more is rejected by the Python wrapper's struct as by the check
    q, keep3 = L.seq_ctl(breakers=range(1025))
    lg = np.zeros(2000, np.float32)
    assert L.lib().xh_seq_adjust_host(L.ptr(lg), 2000, ctypes.byref(q), None, 0, None, None, None) == 1
    del keep, keep2, keep3


# ---- DRY and the ban on the host -------------------------------------------------------------------
@pytest.mark.parametrize("V", Q.VOCABS)
def test_seq_adjust_host_grid_bitwise(V):
    lg = Q.logits(V)
    touched = banned = 0
    for n, kw in Q.dry_grid():
        kw = Q.grid_controls(V, kw)
        win = Q.grid_window(V, 1100)[:n]
        want, rep, ng = Q.seq_adjust(lg, win, **kw)
        out, r, g = L.seq_adjust_host(lg, win, **kw)
        assert np.array_equal(r, rep) and np.array_equal(g, ng), (V, n, kw)
        assert np.array_equal(bits(out), bits(want)), (V, n, kw)
        touched += int((bits(want) != bits(lg)).sum())
        banned += int(np.isneginf(want).sum())
    assert touched > banned > 0                # the grid exercises both stages


@pytest.mark.parametrize("name", sorted(Q.edge_cases()))
def test_seq_adjust_host_edge_case(name):
    V, lg, win, seq, ctl, expect = Q.edge_cases()[name]
    lp = X.adjust(lg, win, **ctl)
    want, rep, ng = Q.edge_expected(name)
    out, r, g = L.seq_adjust_host(lp, win, **seq)
    assert np.array_equal(r, rep) and np.array_equal(g, ng), name
    assert np.array_equal(bits(out), bits(want)), name
    if expect is not None:
        assert {int(c): (int(rep[c]), int(ng[c])) for c in np.flatnonzero(ng)} == expect, name


def test_edge_cases_mean_what_their_names_say():
    E = Q.edge_cases()
    F = np.float32

    def one(name):
        V, lg, win, seq, ctl, _ = E[name]
        return X.adjust(lg, win, **ctl), Q.edge_expected(name)[0], seq
    lp, out, _ = one("below_allowed")
    assert np.array_equal(bits(lp), bits(out))                          # untouched: the bits kept
    lp, out, seq = one("at_allowed")
    assert out[9] == F(lp[9] - F(seq["dry_multiplier"])) and (bits(out) != bits(lp)).sum() == 1
    lp, out, _ = one("breaker_last")
    assert np.array_equal(bits(lp), bits(out))                          # no DRY at all
    lp, out, seq = one("breaker_in_suffix")
    assert np.array_equal(bits(lp), bits(out))                          # dry_9 = 1 < 2, although raw_9 = 3
    lp, out, _ = one("bias_neg_inf")
    assert np.isneginf(lp[9]) and np.isneginf(out[9]) and (bits(out) != bits(lp)).sum() == 0
    lp, out, seq = one("in_penalty_window")
    raw = E["in_penalty_window"][1]
    assert lp[9] != raw[9] and out[9] == F(lp[9] - F(F(seq["dry_multiplier"]) * F(seq["dry_base"])))
    lp, out, _ = one("overflow")
    assert np.isfinite(lp[9]) and np.isneginf(out[9])
    lp, out, _ = one("match_cap")
    assert np.isfinite(out[9]) and out[9] < lp[9]
    lp, out, _ = one("ngram_2")
    assert np.flatnonzero(np.isneginf(out)).tolist() == [8, 9]
    lp, out, _ = one("ngram_64")
    assert np.isneginf(out).sum() == 1
    lp, out, _ = one("ngram_longer_than_window")
    assert np.array_equal(bits(lp), bits(out))
    for name in ("window_1023", "window_1024", "window_over_ring"):
        lp, out, _ = one(name)
        assert (bits(out) != bits(lp)).sum() == 1, name
    lg, win, seq, ctl = Q.empty_vocabulary_case()
    out, _, _ = Q.seq_adjust(X.adjust(lg, win, **ctl), win, **seq)
    assert np.isneginf(out).all()
    assert np.isneginf(L.seq_adjust_host(X.adjust(lg, win, **ctl), win, **seq)[0]).all()


# ---- XTC on the host -------------------------------------------------------------------------------
def check_xtc_host(an, lg, t, th, case):
    undecided = 0
    for i in range(R.N_DRAWS):
        pos = R.POS0 + i
        fired = an.fired(R.SEED, pos)
        kept, n, f = L.xtc_host(lg, t, an.off.kept_map, R.SEED, pos, xtc_probability=an.prob, xtc_threshold=th)
        assert f == fired, (case, i)
        if not an.decided(fired):
            undecided += 1
            continue
        want, _, _ = an.view(fired)
        assert np.array_equal(kept, want) and n == int(want.sum()), (case, i)
    return undecided


@pytest.mark.parametrize("V", Q.VOCABS)
def test_xtc_host_grid_and_skip_cap(V):
    lg = Q.logits(V)
    skipped = fired_some = 0
    for case in Q.xtc_grid():
        t, k, ty, p, pr, th = case
        an = Q.xtc_analysis(V, *case)
        if not (an.decided(True) and an.decided(False)):
            skipped += 1
            continue
        assert check_xtc_host(an, lg, t, th, (V,) + case) == 0
        fired_some += an.n_a >= 2
    assert skipped <= R.SKIP_CAP * len(Q.xtc_grid()), skipped
    assert fired_some >= len(Q.xtc_grid()) // 4


@pytest.mark.parametrize("name", sorted(Q.xtc_edge_cases()))
def test_xtc_host_edge_case(name):
    lg, kw, n_a, kept_ids = Q.xtc_edge_cases()[name]
    an = Q.xtc_edge_analysis(name)
    assert an.decided(True) and an.decided(False), (name, an.reasons, an.off.reasons)
    if n_a is not None:
        assert an.n_a == n_a
    if kept_ids is not None:
        assert np.flatnonzero(an.kept_on).tolist() == kept_ids
    assert check_xtc_host(an, lg, kw["temperature"], kw["xtc_threshold"], name) == 0
    fires = [an.fired(R.SEED, R.POS0 + i) for i in range(R.N_DRAWS)]
    if kw["xtc_probability"] == 1.0:
        assert all(fires)
    else:   # per xh_philox4x32's word 1 some of the draws fire and some do not
        u = [(int(L.philox4x32(R.SEED, R.POS0 + i)[1]) >> 8) * 2.0 ** -24 for i in range(R.N_DRAWS)]
        assert fires == [x < kw["xtc_probability"] for x in u] and 0 < sum(fires) < R.N_DRAWS
    if name == "behind_typical":
        order = np.argsort(-lg, kind="stable")
        c = np.flatnonzero(an.off.kept_map)
        assert not np.array_equal(np.sort(order[:c.size]), c) and an.n_a >= 2   # C is no prefix
    if name == "top_p_behind":
        assert an.n_a >= 2 and an.final_on.n_kept < int(an.kept_on.sum())
