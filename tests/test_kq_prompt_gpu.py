"""XH_OPT_PREFILL_KQ: the K-quant prompt GEMM (gemm_kq.h) through xh_op_prompt_matmul_kq against float64 and
the dequantised weights, and whole passes against the oracle's token loop over the dequantised rows.
Tile: 256 weight rows x 128 tokens, 32-deep K steps, slices of whole 256-element super-blocks."""
import numpy as np
import pytest

import kq_ref as R
import prompt_gemm_ref as G
from bars import check_logp, north
from oracle import oracle as O
from test_kq_gpu import every_code_matrix, kq_files, oracle_from_xalm  # noqa: F401 (kq_files: a fixture)
from test_kq_prompt_cpu import E_INVALID
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model

pytestmark = pytest.mark.gpu

DTYPES = [L.Q4_K, L.Q6_K]
BR, BT = 256, 128


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# (rows, n, K, ks): every edge of the tiling once, a few combinations
CASES = [(1, 1, 256, 0), (BR - 1, BT - 1, 512, 2), (BR, BT, 768, 1), (BR + 32, BT + 1, 512, 0), (BR + 32, 1, 768, 0),
         (1, BT + 1, 256, 1), (BR, BT - 1, 2048, 8)]


@pytest.mark.parametrize("rows,n,K,ks", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_against_float64(dtype, rows, n, K, ks):
    rng = np.random.default_rng(rows * 7 + n * 3 + K + dtype)
    w = R.random_blocks(dtype, rows * (K // 256), rng).reshape(rows, -1)
    x = G.random_x(rng, n, K)
    y = L.op_prompt_matmul_kq(x, w, dtype, rows, ks)
    x64 = x.astype(np.float64)
    err = np.abs(y - x64 @ R.dequantize(dtype, w).astype(np.float64).T)
    bound = 1e-5 * (np.abs(x64) @ R.terms(dtype, w).T) + 1e-7
    print(f"dtype {dtype} rows {rows} n {n} K {K} ks {ks}: worst err / bar {float((err / bound).max()):.3g}")
    assert np.all(err <= bound)
    assert np.array_equal(bits(y), bits(L.op_prompt_matmul_kq(x, w, dtype, rows, ks)))


@pytest.mark.parametrize("ks", [0, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_hot_probes_return_the_weights(dtype, ks):
    w = every_code_matrix(dtype).reshape(64, -1)
    want = 2.0 * R.dequantize(dtype, w)  # [64][512]
    for c0 in range(0, 512, BT):
        x = np.zeros((BT, 512), np.float32)
        x[np.arange(BT), c0 + np.arange(BT)] = 2.0
        y = L.op_prompt_matmul_kq(x, w, dtype, 64, ks)
        assert np.array_equal(bits(y), bits(want[:, c0:c0 + BT].T + np.float32(0))), (dtype, ks, c0)


@pytest.mark.parametrize("dtype,rows,K,n,ks,null_x", [(L.Q4_K, 8, 128, 4, 0, False), (L.Q4_K, 8, 256, 0, 0, False),
                                                      (L.Q6_K, 8, 256, 2049, 0, False), (L.Q6_K, 0, 256, 4, 0, False),
                                                      (L.Q4_K, 8, 768, 4, 3, False), (L.Q4_K, 8, 256, 4, 16, False),
                                                      (L.Q4_0, 8, 256, 4, 0, False), (L.Q6_K, 8, 256, 4, 0, True)])
def test_invalid_arguments_leave_y_untouched(dtype, rows, K, n, ks, null_x):
    y = np.full((8, 8), 7.5, dtype=np.float32)
    x, w = np.ones((4, 768), np.float32), np.ones((8, 3 * 210), np.uint8)
    rc = L.lib().xh_op_prompt_matmul_kq(L.ptr(y), None if null_x else L.ptr(x), L.ptr(w), dtype, rows, K, n, ks)
    assert rc == E_INVALID and np.all(y == 7.5)


# ---- whole passes ---------------------------------------------------------------------------------
N_TOK, N_SCORED = 100, 70
_ORACLE = {}


def toks_of(vocab):
    return [1] + [3 + (i * 37) % (vocab - 3) for i in range(N_TOK - 1)]


def oracle_logits(xf, t, toks):
    """the token loop's logits at every position, once per file"""
    if t not in _ORACLE:
        om = oracle_from_xalm(xf)
        lgs = []
        for pos, tok in enumerate(toks):
            om.forward(tok, pos)
            lgs.append(om.logits().copy())
        om.close()
        _ORACLE[t] = lgs
    return _ORACLE[t]


@pytest.mark.parametrize("option", [1, 0])
@pytest.mark.parametrize("t", ["q4_k_m", "q4_k", "q6_k"])
def test_passes_match_the_token_loop(kq_files, t, option):
    gm = Model.from_xalm(kq_files[t])
    gm.set_option(L.OPT_PREFILL_KQ, option)
    assert gm.get_option(L.OPT_PREFILL_KQ) == option
    toks = toks_of(gm.config.vocab_size)
    assert gm.prefill_route(N_TOK, 0) == (N_TOK, 1 if option else 2)
    lgs = oracle_logits(kq_files[t], t, toks)
    st = InferenceState(gm.config)
    gm.prefill(toks, 0, st)
    err = float(np.abs(st.logits() - lgs[-1]).max())
    assert err <= north(lgs[-1]), (t, option, err, north(lgs[-1]))
    gm.reset()
    got = gm.token_probs(toks[:N_SCORED])
    for pos in range(N_SCORED - 1):
        ref_p = O.sample_prob(lgs[pos], toks[pos + 1])
        if ref_p < 1e-30:
            assert got[pos] < 1e-30
            continue
        check_logp(float(abs(np.log(got[pos]) - np.log(ref_p))), lgs[pos], None, pos)
    gm.close()


def test_f16_model_ignores_the_option():
    from test_forward_gpu import synthetic_pair
    out = []
    for option in (0, 1):
        gm, _om = synthetic_pair(L.F16)
        gm.set_option(L.OPT_PREFILL_KQ, option)
        st = InferenceState(gm.config)
        gm.prefill(toks_of(gm.config.vocab_size), 0, st)
        out.append(bits(st.logits()).copy())
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("bad", [2, -1])
def test_option_values(kq_files, bad):
    gm = Model.from_xalm(kq_files["q4_k"])
    gm.set_option(L.OPT_PREFILL_KQ, 1)
    with pytest.raises(L.XhError):
        gm.set_option(L.OPT_PREFILL_KQ, bad)
    assert gm.get_option(L.OPT_PREFILL_KQ) == 1
    gm.close()
