"""The top-N log-probabilities without a GPU: xh_top_logprobs_host against the numpy reference
(ids and ranks exactly, log-probabilities within logprob_bound) over the shared case list, the
invalid-argument list before the device is touched, and the new exports of the C ABI."""
import ctypes

import numpy as np
import pytest

import top_logprobs_ref as T
from xalm_amd import _lib as L

NEW_EXPORTS = ("xh_top_logprobs_host", "xh_op_top_logprobs", "xh_set_top_logprobs", "xh_get_top_logprobs", "xh_score")


@pytest.mark.parametrize("n_rows", T.N_ROWS)
@pytest.mark.parametrize("V", T.VOCABS)
def test_host_matches_reference(V, n_rows):
    for name, (lg, tg) in T.cases(V, n_rows).items():
        for n_top in T.N_TOPS:
            got = L.top_logprobs_host(lg, n_top, tg)
            T.check_rows(lg, n_top, tg, got, (name, V, n_top))
            # without targets: the same lists
            ids, lps = L.top_logprobs_host(lg, n_top)
            assert (ids == got[0]).all() and (lps.view(np.uint32) == got[1].view(np.uint32)).all(), (name, V, n_top)


def test_cases_cover_what_they_name():
    V = 1025
    c = T.cases(V, 3)
    lg, tg = c["all_equal"]
    ids, lp, tlp, rank = T.top(lg[0], 5, int(tg[0]))
    assert ids.tolist() == [0, 1, 2, 3, 4] and rank == V - 1          # the lowest indices win; rank = index
    lg, tg = c["tie_block"]
    for r in range(3):
        blk = np.flatnonzero(lg[r] == np.float32(5.5))
        assert blk.size == 40 and (lg[r] > 5.5).sum() == 3 and tg[r] in blk
        ids, _ = T.top(lg[r], 5)
        assert ids[3:].tolist() == blk[:2].tolist()                   # the cut is inside the block
        assert T.top(lg[r], 5, int(tg[r]))[3] == 3 + int(np.flatnonzero(blk == tg[r])[0])
    lg, tg = c["signed_zeros"]
    o = T.order(lg[1])
    assert not np.signbit(lg[1][o[:20]]).any() and (lg[1][o[:20]] == 0).all()  # +0 first ...
    assert np.signbit(lg[1][o[20:40]]).all() and (lg[1][o[20:40]] == 0).all()  # ... then -0
    lg, tg = c["peaked_digit"]
    assert np.unique(T.keys(lg[0]) >> np.uint64(24)).size == 1
    lg, tg = c["mostly_neg_inf"]
    ids, lp, tlp, rank = T.top(lg[0], 5, int(tg[0]))
    assert np.isfinite(lp[:3]).all() and np.isneginf(lp[3:]).all() and np.isneginf(tlp)
    neg = np.flatnonzero(np.isneginf(lg[0]))
    assert ids[3:].tolist() == neg[:2].tolist() and rank == 3          # the first -inf token follows the finite three
    lg, tg = T.cases(V, 1)["normal"]
    assert T.top(lg[0], 1, int(tg[0]))[3] == 0                        # a target that is the maximum


def _call(fn, lg, V, rows, n_top, tg, ids, lps, tlp, rank):
    p = lambda a: None if a is None else L.ptr(a)  # noqa: E731
    return fn(p(lg), V, rows, n_top, p(tg), p(ids), p(lps), p(tlp), p(rank))


@pytest.mark.parametrize("entry", ("xh_top_logprobs_host", "xh_op_top_logprobs"))
def test_invalid_arguments(entry):
    """XH_E_INVALID before any work; for the device entry, before the device is touched (this test
    has no GPU)."""
    fn = getattr(L.lib(), entry)
    V, rows = 300, 2
    lg = np.zeros((rows, V), dtype=np.float32)
    tg = np.array([0, V - 1], dtype=np.int32)
    ids = np.zeros((rows, 32), dtype=np.int32)
    lps = np.zeros((rows, 32), dtype=np.float32)
    tlp = np.zeros(rows, dtype=np.float32)
    rank = np.zeros(rows, dtype=np.int32)
    ok = dict(lg=lg, V=V, rows=rows, n_top=5, tg=tg, ids=ids, lps=lps, tlp=tlp, rank=rank)
    bad = {
        "n_top_0": dict(n_top=0), "n_top_negative": dict(n_top=-1), "n_top_33": dict(n_top=L.TOP_MAX + 1),
        "null_logits": dict(lg=None), "null_ids": dict(ids=None), "null_lps": dict(lps=None),
        "vocab_0": dict(V=0), "vocab_over_2_17": dict(V=(1 << 17) + 1), "rows_0": dict(rows=0),
        "target_negative": dict(tg=np.array([0, -1], dtype=np.int32)),
        "target_vocab": dict(tg=np.array([V, 0], dtype=np.int32)),
        "targets_without_outputs": dict(tlp=None, rank=None), "outputs_without_targets": dict(tg=None),
        "rank_alone_missing": dict(rank=None),
    }
    for name, change in bad.items():
        assert _call(fn, **dict(ok, **change)) == 1, name
    # n_top may not exceed the vocabulary
    small = np.zeros((1, 4), dtype=np.float32)
    assert _call(fn, small, 4, 1, 5, None, ids, lps, None, None) == 1
    if entry == "xh_top_logprobs_host":
        assert _call(fn, **ok) == 0
        assert _call(fn, small, 4, 1, 4, None, ids, lps, None, None) == 0


def test_context_entries_reject_null():
    lib = L.lib()
    assert lib.xh_set_top_logprobs(None, 5) == 1
    assert lib.xh_get_top_logprobs(None, 1, None, None, None) == 1
    toks = np.array([1, 2, 3], dtype=np.int32)
    assert lib.xh_score(None, L.ptr(toks), 3, 0, 0, None, None, None, None, None) == 1


def test_new_symbols_are_exported():
    lib = ctypes.CDLL(L.HIP_LIB_PATH)
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert name in L._SIGNATURES, name
