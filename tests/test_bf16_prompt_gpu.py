"""XH_OPT_PREFILL_BF16: the bf16-weight prompt GEMM (gemm_bf16.h) and its piece producer through
xh_op_prompt_matmul_bf16, against float64 and the exact cases of prompt_gemm_ref.py, and whole passes
against the oracle's token loop.  Tile: 256 weight rows x 128 tokens, 32-deep K steps, slices of 64s.

Exactness of the sparse sums on this route (checked below on the inputs themselves): x = m u with m an
integer below 2^22, so every piece is an integer multiple of u, and sum_k |w_k| (|b0| + |b1| + |b2|)
< 2^24 u: every product and every partial sum in any order is exact in f32."""
import functools

import numpy as np
import pytest

import prompt_gemm_ref as R
from oracle import oracle as O
from test_bf16_prompt_cpu import E_INVALID, bf16_pieces, bf16_val
from test_forward_gpu import check, check_probs, synthetic_pair
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState

pytestmark = pytest.mark.gpu

BR, BT = 256, 128


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def w16(w):
    return np.ascontiguousarray(w).view(np.uint16)


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("K", [64, 192])
def test_pieces_are_the_numpy_split(n, K):
    rng = np.random.default_rng(K + n)
    x = R.random_x(rng, n, K)  # both signs, rows scaled 2^-20 .. 2^20: second and third pieces non-zero
    x[:, ::7] = 0.0
    x[0, 1] = -0.0
    _y, pieces = L.op_prompt_matmul_bf16(x, w16(R.random_weights(rng, L.BF16, 8, K)))
    want = bf16_pieces(x)
    assert (want[1] != 0).any() and (want[2] != 0).any()
    assert np.array_equal(pieces, want)


# (rows, n, K, ks, wide): every edge of the tiling once, a few combinations; wide = weights over 2^-30 .. 2^20
CASES = [(1, 1, 64, 0, False), (BR - 1, BT - 1, 128, 2, False), (BR, BT, 448, 1, False), (BR + 32, BT + 1, 128, 0, False),
         (BR + 32, 1, 448, 0, False), (1, BT + 1, 128, 1, False), (BR, BT - 1, 64, 1, False), (BR + 32, BT + 1, 448, 0, True)]


@pytest.mark.parametrize("rows,n,K,ks,wide", CASES)
def test_gemm_against_float64(rows, n, K, ks, wide):
    rng = np.random.default_rng(rows * 7 + n * 3 + K)
    x = R.random_x(rng, n, K)
    if wide:  # weights over 2^-30 .. 2^20: no f16 image could hold them
        v = (rng.standard_normal((rows, K)) * np.exp2(rng.integers(-30, 21, size=(rows, K)))).astype(np.float32)
        w = R.from_values(L.BF16, v)
    else:
        w = R.random_weights(rng, L.BF16, rows, K)
    W = R.decode_weights(L.BF16, w, rows, K)
    y, _ = L.op_prompt_matmul_bf16(x, w16(w), ks)
    x64 = x.astype(np.float64)
    err = np.abs(y - x64 @ W.T)
    bound = 1e-5 * (np.abs(x64) @ np.abs(W).T) + 1e-7
    print(f"rows {rows} n {n} K {K} ks {ks}: worst err / bound {float((err / bound).max()):.3g}")
    assert np.all(err <= bound)
    y2, _ = L.op_prompt_matmul_bf16(x, w16(w), ks)
    assert np.array_equal(bits(y), bits(y2))


@pytest.mark.parametrize("K,ks", [(128, 2), (448, 1), (256, 0)])
def test_one_hot_probes_return_the_weights(K, ks):
    rows = BR + 16
    kl = R.probe_ks(K, 8, max(ks, 1))
    w = R.coded_weights(L.BF16, rows, K, False)
    y, _ = L.op_prompt_matmul_bf16(R.probe_x(kl, K), w16(w), ks)
    want = R.decode_weights(L.BF16, w, rows, K)[:, kl].T.astype(np.float32) + np.float32(0)
    assert np.array_equal(bits(y), bits(want))


@pytest.mark.parametrize("rows,n,K,ks", [(BR + 32, BT + 1, 128, 2), (40, 5, 448, 0)])
def test_sparse_sums_are_exact(rows, n, K, ks):
    x, w, v, units = R.sparse_case(np.random.default_rng(rows + K), L.BF16, rows, K, n)
    assert R.exact_terms_ok(x, v, units)
    p = np.abs(bf16_val(bf16_pieces(x)).astype(np.float64)) / units[None, :, None]
    assert np.array_equal(p, np.round(p)) and (p[2] != 0).any(axis=1).all()
    assert np.all(p.sum(axis=0) @ np.abs(v).T.astype(np.float64) < 2 ** 24)
    y, _ = L.op_prompt_matmul_bf16(x, w16(w), ks)
    assert np.array_equal(bits(y), bits((x.astype(np.float64) @ v.T.astype(np.float64)).astype(np.float32)))


@pytest.mark.parametrize("rows,K,n,ks,null_x", [(8, 128, 4, 3, False), (8, 192, 4, 2, False), (8, 1024, 4, 16, False),
                                                (8, 96, 4, 0, False), (8, 128, 0, 0, False), (8, 128, 2049, 0, False),
                                                (0, 128, 4, 0, False), (8, 128, 4, -1, False), (8, 128, 4, 0, True)])
def test_invalid_arguments_leave_y_untouched(rows, K, n, ks, null_x):
    y = np.full((8, 8), 7.5, dtype=np.float32)
    x, w = np.ones((4, 1024), np.float32), np.ones((8, 1024), np.uint16)
    rc = L.lib().xh_op_prompt_matmul_bf16(L.ptr(y), None if null_x else L.ptr(x), L.ptr(w), rows, K, n, ks, None)
    assert rc == E_INVALID and np.all(y == 7.5)


# ---- whole passes ---------------------------------------------------------------------------------
TOKS = [1] + [3 + (i * 37) % 500 for i in range(99)]


def pair(wdt, option, cls_bf16=False):
    gm, om = synthetic_pair(wdt)
    if cls_bf16:
        gm.upload_synthetic(L.WCLS, 0, L.BF16, 12, 0.0, 0.05)
        om.set_tensor(L.WCLS, 0, L.BF16, O.synthetic(gm.config.vocab_size, gm.config.dim, L.BF16, 12, 0.0, 0.05))
    gm.set_option(L.OPT_PREFILL_BF16, option)
    assert gm.get_option(L.OPT_PREFILL_BF16) == option
    return gm, om


@functools.lru_cache(maxsize=None)
def oracle_logits():
    _gm, om = synthetic_pair(L.BF16)
    for pos, tok in enumerate(TOKS):
        om.forward(tok, pos, L.OUTPUT_LOGITS if pos == len(TOKS) - 1 else L.HYDRATE_KV_CACHE)
    return om.logits().copy()


@pytest.mark.parametrize("option", [1, 0])
def test_passes_match_the_token_loop(option):
    gm, _om = pair(L.BF16, option)
    assert gm.prefill_route(len(TOKS), 0) == (len(TOKS), 1 if option else 2)
    st = InferenceState(gm.config)
    gm.prefill(TOKS, 0, st)
    check(st.logits(), oracle_logits())


def test_token_probs_with_a_bf16_lm_head():
    gm, om = pair(L.BF16, 1, cls_bf16=True)
    check_probs(gm.token_probs(TOKS[:70]), om, TOKS[:70])


def test_f16_model_ignores_the_option():
    out = []
    for option in (0, 1):
        gm, _om = pair(L.F16, option)
        st = InferenceState(gm.config)
        gm.prefill(TOKS, 0, st)
        out.append(bits(st.logits()).copy())
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("bad", [2, -1])
def test_option_values(bad):
    gm, _om = pair(L.BF16, 1)
    with pytest.raises(L.XhError):
        gm.set_option(L.OPT_PREFILL_BF16, bad)
    assert gm.get_option(L.OPT_PREFILL_BF16) == 1
