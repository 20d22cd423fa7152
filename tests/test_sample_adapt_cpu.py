"""The adaptive draw without a GPU: the new symbols, parameter validation before the device is
touched, xh_truncate_host against the reference on the case lists, the host Sampler's route with the
new controls off, and the skip cap of the GPU tests' case lists on the reference alone."""
import ctypes
import os

import numpy as np
import pytest

import sample_adapt_ref as A
import sample_ext_ref as X
import sample_ref as R
from conftest import ROOT
from xalm_amd import _lib as L

HOST_SO = os.path.join(ROOT, "xalm_amd", "lib", "libxalm_host.so")
NAN, INF = float("nan"), float("inf")


def test_symbols_exported():
    lib = L.lib()
    for name in ("xh_decode_sample_adapt", "xh_op_sample_adapt", "xh_truncate_host"):
        assert hasattr(lib, name), name
    import xalm_amd
    assert callable(xalm_amd.op_sample_adapt) and hasattr(xalm_amd.Model, "decode_sample_adapt")
    assert hasattr(ctypes.CDLL(HOST_SO), "xalm_sample_adapt")


# (xh_trunc_ctl fields, sampling overrides, min_p, mu)
BAD = [
    (dict(typical_p=0.0), {}, 0.0, 0.0), (dict(typical_p=-0.5), {}, 0.0, 0.0), (dict(typical_p=1.5), {}, 0.0, 0.0),
    (dict(typical_p=NAN), {}, 0.0, 0.0),
    (dict(top_n_sigma=-1.0), {}, 0.0, 0.0), (dict(top_n_sigma=INF), {}, 0.0, 0.0), (dict(top_n_sigma=NAN), {}, 0.0, 0.0),
    (dict(mirostat_tau=-1.0), {}, 0.0, 0.0), (dict(mirostat_tau=INF), {}, 0.0, 0.0), (dict(mirostat_tau=NAN), {}, 0.0, 0.0),
    (dict(mirostat_tau=3.0, mirostat_eta=0.0), {}, 0.0, 6.0), (dict(mirostat_tau=3.0, mirostat_eta=-0.1), {}, 0.0, 6.0),
    (dict(mirostat_tau=3.0, mirostat_eta=INF), {}, 0.0, 6.0), (dict(mirostat_tau=3.0, mirostat_eta=NAN), {}, 0.0, 6.0),
    (dict(mirostat_tau=3.0), {}, 0.0, -1.0), (dict(mirostat_tau=3.0), {}, 0.0, INF), (dict(mirostat_tau=3.0), {}, 0.0, NAN),
    (dict(mirostat_tau=3.0), dict(top_k=40), 0.0, 6.0), (dict(mirostat_tau=3.0), dict(top_p=0.9), 0.0, 6.0),
    (dict(mirostat_tau=3.0), {}, 0.05, 6.0), (dict(mirostat_tau=3.0, typical_p=0.9), {}, 0.0, 6.0),
    (dict(mirostat_tau=3.0, top_n_sigma=1.0), {}, 0.0, 6.0),
]


def trunc(typical_p=1.0, top_n_sigma=0.0, mirostat_tau=0.0, mirostat_eta=0.1):
    return L.XhTruncCtl(typical_p, top_n_sigma, mirostat_tau, mirostat_eta)


def call_all(t, s, c, mu, hist=None, n_hist=0, constrain=0):
    """(xh_decode_sample_adapt with a null context, xh_op_sample_adapt, xh_truncate_host) return codes."""
    lib = L.lib()
    V = 64
    lg = np.zeros(V, np.float32)
    toks, kept = np.zeros(4, np.int32), np.zeros(4, np.int32)
    st, mus = np.zeros(4, np.uint32), np.zeros(4, np.float32)
    done = ctypes.c_int(-1)
    tp = ctypes.byref(t) if t is not None else None
    cp = ctypes.byref(c) if c is not None else None
    sp = ctypes.byref(s) if s is not None else None
    a = lib.xh_decode_sample_adapt(None, 0, 4, sp, cp, tp, hist, n_hist, constrain, 0, mu, -1, -1, L.ptr(toks), None, None,
                                   None, ctypes.byref(done))
    assert done.value == 0
    b = lib.xh_op_sample_adapt(L.ptr(lg), V, sp, cp, tp, hist, n_hist, None, None, None, 0, mu, -1, -1, 0, 4, L.ptr(toks),
                               L.ptr(kept), L.ptr(st), L.ptr(mus), None, None)
    h = lib.xh_truncate_host(L.ptr(lg), V, sp, c.min_p if c is not None else 0.0, tp, mu, -1, None, None, None, None)
    return a, b, h


@pytest.mark.parametrize("case", BAD, ids=[str(i) for i in range(len(BAD))])
def test_invalid_trunc_rejected_before_the_device(case):
    tkw, skw, min_p, mu = case
    s = L.XhSampling(1.0, skw.get("top_k", 0), skw.get("top_p", 1.0), 1)
    c, keep = L.logit_ctl(min_p=min_p)
    assert call_all(trunc(**tkw), s, c, mu) == (1, 1, 1)
    assert L.lib().xh_last_error(None)
    del keep


def test_invalid_composed_arguments_rejected():
    """A null xh_trunc_ctl, and every invalid argument of the loops this one composes."""
    good = L.XhSampling(1.0, 0, 1.0, 1)
    c, keep = L.logit_ctl()
    assert call_all(None, good, c, 0.0) == (1, 1, 1)
    for bad in (L.XhSampling(-1.0, 0, 1.0, 1), L.XhSampling(NAN, 0, 1.0, 1), L.XhSampling(1.0, -1, 1.0, 1),
                L.XhSampling(1.0, 0, 0.0, 1), L.XhSampling(1.0, 0, 1.5, 1), None):
        assert call_all(trunc(), bad, c, 0.0)[:2] == (1, 1)
    assert call_all(trunc(), L.XhSampling(0.0, 0, 1.0, 1), c, 0.0)[2] == 1  # greedy truncates nothing: no host set
    for kw in (dict(repeat_penalty=0.0), dict(presence_penalty=NAN), dict(last_n=1025), dict(min_p=1.5),
               dict(logit_bias=[(3, 1.0), (3, 2.0)]), dict(logit_bias=[(-1, 1.0)]), dict(logit_bias=[(3, NAN)])):
        cb, kb = L.logit_ctl(**kw)
        assert call_all(trunc(), good, cb, 0.0)[:2] == (1, 1), kw
        del kb
    win = np.array([1, 2, 3], np.int32)
    c3, k3 = L.logit_ctl(last_n=3)
    assert call_all(trunc(), good, c3, 0.0, L.ptr(win), -1)[:2] == (1, 1)
    assert call_all(trunc(), good, c3, 0.0, None, 3)[:2] == (1, 1)
    neg = np.array([1, -2, 3], np.int32)
    assert call_all(trunc(), good, c3, 0.0, L.ptr(neg), 3)[:2] == (1, 1)
    # constrain without a context cannot have its uploads
    assert call_all(trunc(), good, c, 0.0, constrain=1)[0] == 1
    # a valid call still fails without a context, and the op and the host function accept it up to the device
    assert call_all(trunc(typical_p=0.9, top_n_sigma=1.0), good, None, 0.0)[2] == 0
    del keep, k3


def host(an_kw, lg, token=-1):
    kw = dict(an_kw)
    return L.truncate_host(lg, kw.pop("temperature"), top_k=kw.get("top_k", 0), top_p=kw.get("top_p", 1.0),
                           min_p=kw.get("min_p", 0.0), typical_p=kw.get("typical_p", 1.0),
                           top_n_sigma=kw.get("top_n_sigma", 0.0), mirostat_tau=kw.get("tau", 0.0),
                           mirostat_eta=kw.get("eta", 0.1), mu=kw.get("mu", 0.0), token=token)


def check_host(an, kw, lg, name):
    kept, n, thr, _ = host(kw, lg)
    assert np.array_equal(kept, an.kept_map), (name, np.flatnonzero(kept != an.kept_map)[:8])
    assert n == int(an.kept_map.sum()), name
    if np.isfinite(an.thr):
        assert abs(thr - an.thr) <= float(np.spacing(np.float32(abs(an.thr)))), (name, thr, an.thr)
    else:
        assert thr == an.thr, name
    if an.K is not None:
        for tok in np.flatnonzero(an.kept_map)[:4]:
            if an.M[tok] == 0:
                continue
            want, obs = an.mu_next(int(tok))
            got = host(kw, lg, int(tok))[3]
            assert abs(got - want) <= A.mu_bound(an.mu, obs, an.tau), (name, tok, got, want)


@pytest.mark.parametrize("V", A.VOCABS)
def test_truncate_host_matches_reference_on_the_grids(V):
    lg = R.peaked_logits(V)
    for (t, k, ty, ns, p) in A.grid():
        an = A.grid_analysis(V, t, k, ty, ns, p)
        if an.decided:
            check_host(an, dict(temperature=t, top_k=k, top_p=p, typical_p=ty, top_n_sigma=ns), lg, (t, k, ty, ns, p))
    for (t, tau, eta, mu) in A.miro_grid():
        an = A.miro_analysis(V, t, tau, eta, mu)
        if an.decided:
            check_host(an, dict(temperature=t, tau=tau, eta=eta, mu=mu), lg, (t, tau, eta, mu))


def test_truncate_host_matches_reference_on_the_edge_cases():
    for name, (lg, kw, ctl, kept) in A.edge_cases().items():
        an = A.edge_analysis(name)
        check_host(an, kw, X.adjust(lg, (), **ctl), name)


@pytest.mark.parametrize("V", A.VOCABS)
def test_skip_cap_on_reference(V):
    grid = A.grid()
    undecided = [(c, A.grid_analysis(V, *c).reasons) for c in grid if not A.grid_analysis(V, *c).decided]
    assert len(undecided) <= R.SKIP_CAP * len(grid), undecided
    mg = A.miro_grid()
    undecided = [(c, A.miro_analysis(V, *c).reasons) for c in mg if not A.miro_analysis(V, *c).decided]
    assert len(undecided) <= R.SKIP_CAP * len(mg), undecided
    # the stages move the kept set
    assert A.grid_analysis(V, 1.5, 0, 0.2, 0.0, 1.0).n_kept <= A.grid_analysis(V, 1.5, 0, 0.9, 0.0, 1.0).n_kept < V
    assert A.grid_analysis(V, 1.5, 0, 0.9, 0.0, 1.0).n_kept > 1
    assert 1 <= A.grid_analysis(V, 1.5, 0, 1.0, 1.0, 1.0).n_kept < V
    assert A.miro_analysis(V, 1.5, 3.0, 0.1, 2.0).n_kept < A.miro_analysis(V, 1.5, 3.0, 0.1, 10.0).n_kept


def test_edge_cases_reference():
    for name, (lg, kw, ctl, kept) in A.edge_cases().items():
        an = A.edge_analysis(name)
        assert an.decided, (name, an.reasons)
        if kept is not None:
            assert np.flatnonzero(an.kept_map).tolist() == kept, name
        for d in range(8):
            assert an.accepted(R.SEED, R.POS0 + d), name
    an = A.edge_analysis("typical_drops_argmax")
    assert an.kept_map[0] == 0 and int(np.argmax(A.edge_cases()["typical_drops_argmax"][0])) == 0
    assert A.edge_analysis("typical_keeps_one").n_kept == 1
    an = A.edge_analysis("typical_neg_inf_and_massless")
    assert an.kept_map[64:128].sum() == 0 and an.kept_map[130:140].sum() == 0 and (an.M[130:140] == 0).all()
    assert A.edge_analysis("n_sigma_under_top_k").n_kept == 3
    an = A.edge_analysis("min_p_under_n_sigma")
    lg = A.edge_cases()["min_p_under_n_sigma"][0]
    assert an.n_kept == int((lg >= np.float32(an.thr)).sum()) < X.ExtAnalysis(lg, 1.0, 0, 1.0, 1e-9).n_kept
    for name in ("ban_typical", "ban_n_sigma", "ban_mirostat"):
        an = A.edge_analysis(name)
        assert not an.kept_map[[12, 8, 40]].any(), name


def test_host_sampler_reproduces_the_existing_sampler_with_the_new_controls_off():
    lib = ctypes.CDLL(HOST_SO)
    lib.xalm_sample.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(L.XhSampling), ctypes.c_uint64,
                                ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.xalm_sample_adapt.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(L.XhSampling),
                                      ctypes.POINTER(L.XhLogitCtl), ctypes.POINTER(L.XhTruncCtl), ctypes.c_void_p,
                                      ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
    lg = R.peaked_logits(300)
    off = trunc()
    for (t, k, p) in R.grid(300) + [(0.0, 0, 1.0)]:
        s = L.XhSampling(t, k, p, R.SEED)
        for d in range(16):
            old, new, kept, mu = ctypes.c_int(-1), ctypes.c_int(-2), ctypes.c_int(0), ctypes.c_float(-1.0)
            assert lib.xalm_sample(L.ptr(lg), 300, ctypes.byref(s), R.POS0 + d, ctypes.byref(old), ctypes.byref(kept)) == 0
            assert lib.xalm_sample_adapt(L.ptr(lg), 300, ctypes.byref(s), None, ctypes.byref(off), None, 0, R.POS0 + d,
                                         ctypes.byref(mu), ctypes.byref(new)) == 0
            assert new.value == old.value, (t, k, p, d)
            assert mu.value == 0.0  # none given: 2 * tau
    # with a control on the draw follows the reference
    for (t, k, ty, ns, p) in A.grid():
        an = A.grid_analysis(300, t, k, ty, ns, p)
        if not an.decided:
            continue
        s = L.XhSampling(t, k, p, R.SEED)
        tc = trunc(typical_p=ty, top_n_sigma=ns)
        for d in range(8):
            new, mu = ctypes.c_int(-2), ctypes.c_float(-1.0)
            assert lib.xalm_sample_adapt(L.ptr(lg), 300, ctypes.byref(s), None, ctypes.byref(tc), None, 0, R.POS0 + d,
                                         ctypes.byref(mu), ctypes.byref(new)) == 0
            assert new.value in an.accepted(R.SEED, R.POS0 + d), (t, k, ty, ns, p, d)
