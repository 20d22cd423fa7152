"""The extended draw without a GPU: xh_adjust_logits bit for bit against the numpy adjustment,
parameter validation before the device is touched, the host Sampler's route, and the skip cap of the
GPU tests' case lists on the reference alone."""
import ctypes
import os

import numpy as np
import pytest

import sample_ext_ref as X
import sample_ref as R
from conftest import ROOT
from xalm_amd import _lib as L

HOST_SO = os.path.join(ROOT, "xalm_amd", "lib", "libxalm_host.so")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("V", X.ADJ_VOCABS)
def test_adjust_logits_bit_for_bit(V):
    lg = X.adjust_logits_vector(V)
    for name, (win, ctl) in X.adjust_cases(V).items():
        want = X.adjust(lg, win, **ctl)
        got = L.adjust_logits(lg, win, **ctl)
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])


def test_adjust_cases_cover_what_they_name():
    V = 300
    lg = X.adjust_logits_vector(V)
    win, ctl = X.adjust_cases(V)["all_three_bias"]
    out = X.adjust(lg, win, **ctl)
    assert win.count(9) == 3 and {0, V - 1, 5, 6, 7, 8} <= set(win) and not {11, 12} & set(win)
    assert bits(lg)[5] == 0x80000000 and lg[6] == -np.inf and lg[7] > 0 > lg[9]
    assert out[6] == -np.inf and out[8] == -np.inf and out[12] == -np.inf
    assert out[11] == np.float32(lg[11] + np.float32(-2.25))
    # an untouched token keeps its bits, -0 included when it is outside the window
    touched = set(win) | {t for t, _ in X.BIAS}
    keep = np.array([i for i in range(V) if i not in touched])
    assert (bits(out)[keep] == bits(lg)[keep]).all()
    off = X.adjust(lg, [7], last_n=1)
    assert (bits(off) == bits(lg)).all()  # repeat 1, presence 0, frequency 0: a / 1 - c * 0 - 0
    # the three-fold token under all three: one division or product, one product, two differences
    f = np.float32
    assert out[9] == f(f(f(lg[9] * f(1.3)) - f(f(3) * f(0.2))) - f(0.5))
    assert X.adjust(lg, win, **dict(ctl, logit_bias=None))[7] == f(f(f(lg[7] / f(1.3)) - f(0.2)) - f(0.5))


def raw_ctl(**kw):
    c, keep = L.logit_ctl(**{k: v for k, v in kw.items() if k != "raw"})
    for k, v in kw.get("raw", {}).items():
        setattr(c, k, v)
    return c, keep


NAN, INF = float("nan"), float("inf")
BAD_CTL = [
    dict(repeat_penalty=0.0), dict(repeat_penalty=-1.0), dict(repeat_penalty=INF), dict(repeat_penalty=NAN),
    dict(presence_penalty=NAN), dict(presence_penalty=INF), dict(frequency_penalty=NAN), dict(frequency_penalty=-INF),
    dict(last_n=-1), dict(last_n=1025), dict(min_p=1.5), dict(min_p=-0.1), dict(min_p=NAN),
    dict(raw=dict(n_bias=257)), dict(raw=dict(n_bias=-1)), dict(raw=dict(n_bias=2)),  # a count with null arrays
    dict(logit_bias=[(3, 1.0), (3, 2.0)]), dict(logit_bias=[(-1, 1.0)]), dict(logit_bias=[(64, 1.0)]),
    dict(logit_bias=[(3, NAN)]), dict(logit_bias=[(3, INF)]),
]


@pytest.mark.parametrize("kw", BAD_CTL, ids=[str(i) for i in range(len(BAD_CTL))])
def test_invalid_controls_rejected_before_the_device(kw):
    lib = L.lib()
    V = 64
    lg = np.zeros(V, np.float32)
    out = np.zeros(V, np.float32)
    win = np.array([1, 2, 3], np.int32)
    toks = np.zeros(4, np.int32)
    kept = np.zeros(4, np.int32)
    s = L.XhSampling(1.0, 0, 1.0, 1)
    c, keep = raw_ctl(**kw)
    assert lib.xh_adjust_logits(L.ptr(lg), V, ctypes.byref(c), L.ptr(win), 3, L.ptr(out)) == 1
    assert lib.xh_last_error(None)
    assert lib.xh_op_sample_ext(L.ptr(lg), V, ctypes.byref(s), ctypes.byref(c), L.ptr(win), 3, 0, 4, L.ptr(toks),
                                L.ptr(kept), None, None) == 1
    if kw.get("logit_bias") != [(64, 1.0)]:  # without a context the vocabulary is unknown
        done = ctypes.c_int(-1)
        assert lib.xh_decode_sample_ext(None, 0, 4, ctypes.byref(s), ctypes.byref(c), L.ptr(win), 3, -1, -1,
                                        L.ptr(toks), None, ctypes.byref(done)) == 1
        assert done.value == 0
    del keep


def test_invalid_history_and_sampling_rejected():
    lib = L.lib()
    V = 64
    lg = np.zeros(V, np.float32)
    out = np.zeros(V, np.float32)
    win = np.array([1, 2, 3], np.int32)
    toks = np.zeros(4, np.int32)
    kept = np.zeros(4, np.int32)
    s = L.XhSampling(1.0, 0, 1.0, 1)
    c, _ = L.logit_ctl(last_n=3)
    done = ctypes.c_int(-1)
    for hist, n in ((L.ptr(win), -1), (None, 3)):
        assert lib.xh_adjust_logits(L.ptr(lg), V, ctypes.byref(c), hist, n, L.ptr(out)) == 1
        assert lib.xh_op_sample_ext(L.ptr(lg), V, ctypes.byref(s), ctypes.byref(c), hist, n, 0, 4, L.ptr(toks),
                                    L.ptr(kept), None, None) == 1
        assert lib.xh_decode_sample_ext(None, 0, 4, ctypes.byref(s), ctypes.byref(c), hist, n, -1, -1, L.ptr(toks),
                                        None, ctypes.byref(done)) == 1
    oob = np.array([1, V, 3], np.int32)  # a window token outside the vocabulary would index past the logits
    assert lib.xh_adjust_logits(L.ptr(lg), V, ctypes.byref(c), L.ptr(oob), 3, L.ptr(out)) == 1
    assert lib.xh_op_sample_ext(L.ptr(lg), V, ctypes.byref(s), ctypes.byref(c), L.ptr(oob), 3, 0, 4, L.ptr(toks),
                                L.ptr(kept), None, None) == 1
    bad = L.XhSampling(-1.0, 0, 1.0, 1)
    assert lib.xh_op_sample_ext(L.ptr(lg), V, ctypes.byref(bad), None, None, 0, 0, 4, L.ptr(toks), L.ptr(kept), None,
                                None) == 1
    assert lib.xh_decode_sample_ext(None, 0, 4, ctypes.byref(bad), None, None, 0, -1, -1, L.ptr(toks), None,
                                    ctypes.byref(done)) == 1
    # a null ctl is "all off", a valid call: without a context it still fails, but not as a bad control
    assert lib.xh_adjust_logits(L.ptr(lg), V, None, None, 0, L.ptr(out)) == 0
    assert (out == lg).all()


def test_host_sampler_route_unchanged_with_controls_off():
    """xalm_sample (the host Sampler's draw) gives the reference's tokens as before: the min-p
    argument defaults to off."""
    lib = ctypes.CDLL(HOST_SO)
    lib.xalm_sample.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(L.XhSampling), ctypes.c_uint64,
                                ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lg = R.peaked_logits(300)
    for (t, k, p) in R.grid(300):
        an = R.grid_analysis(300, t, k, p)
        if not an.decided:
            continue
        s = L.XhSampling(t, k, p, R.SEED)
        for d in range(16):
            tok, kept = ctypes.c_int(-1), ctypes.c_int(-1)
            assert lib.xalm_sample(L.ptr(lg), 300, ctypes.byref(s), R.POS0 + d, ctypes.byref(tok), ctypes.byref(kept)) == 0
            assert kept.value == an.n_kept and tok.value in an.accepted(R.SEED, R.POS0 + d)
    # all controls off: the adjustment the host Sampler goes through is the identity, bit for bit
    for V in (300, 128256):
        lg = X.adjust_logits_vector(V)
        assert (bits(L.adjust_logits(lg, X.adjust_cases(V)["all_three"][0])) == bits(lg)).all()


@pytest.mark.parametrize("V", R.VOCABS)
def test_skip_cap_on_reference(V):
    grid = X.draw_grid()
    undecided = [c for c in grid if not X.draw_analysis(V, *c).decided]
    assert len(undecided) <= R.SKIP_CAP * len(grid), undecided
    # the controls move the kept set: the window holds the largest logits
    assert not np.array_equal(X.draw_adjusted(V, True), X.draw_adjusted(V, False))
    assert X.draw_analysis(V, 0.7, 0, 1.0, 1.0, False).n_kept == 1  # min_p 1: the maximum alone
    assert 1 <= X.draw_analysis(V, 1.5, 0, 1.0, 0.05, True).n_kept < V


def test_edge_cases_reference():
    for name, (lg, win, t, k, p, ctl, kept) in X.edge_cases().items():
        an = X.edge_analysis(name)
        assert an.decided, name
        if kept is not None:
            assert an.kept.tolist() == kept, name
        for d in range(8):
            assert an.accepted(R.SEED, R.POS0 + d), name
    an = X.edge_analysis("ban_argmax")
    assert all(40 not in an.accepted(R.SEED, R.POS0 + d) for d in range(R.N_DRAWS))
    lg = X.edge_cases()["greedy_demoted"][0]
    assert int(np.argmax(lg)) == 40


def test_logprob_reference():
    lg = R.peaked_logits(300)
    p = np.exp(lg.astype(np.float64) - lg.max())
    p /= p.sum()
    for tok in (0, 17, int(np.argmax(lg))):
        assert abs(X.logprob64(lg, tok) - np.log(p[tok])) < 1e-12
