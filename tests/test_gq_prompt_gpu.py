"""XH_OPT_PREFILL_GQ: the block-code prompt GEMM (gemm_gq.h) through xh_op_prompt_matmul_gq against float64 and
the dequantised weights, and whole passes against the oracle's token loop.
Tile: 256 weight rows x 128 tokens, 32-deep K steps (one block), slices a multiple of 64."""
import numpy as np
import pytest

import gq2_ref as R
import prompt_gemm_ref as G
from bars import check_logp, north
from conftest import fixture_path
from oracle import oracle as O
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

DTYPES = [L.Q8_0, L.Q4_0, L.Q4_1, L.Q5_0, L.Q5_1]
AFFINE = (L.Q4_1, L.Q5_1)
BR, BT = 256, 128


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# (rows, n, K, ks): every edge of the tiling once, a few combinations
CASES = [(1, 1, 64, 0), (BR - 1, BT - 1, 128, 2), (BR, BT, 192, 1), (BR + 32, BT + 1, 128, 0), (BR + 32, 1, 192, 0),
         (1, BT + 1, 64, 1), (BR, BT - 1, 2048, 8)]


@pytest.mark.parametrize("rows,n,K,ks", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_against_float64(dtype, rows, n, K, ks):
    rng = np.random.default_rng(rows * 7 + n * 3 + K + dtype)
    w = G.random_weights(rng, dtype, rows, K)
    x = G.random_x(rng, n, K)
    y = L.op_prompt_matmul_gq(x, w, dtype, rows, ks)
    x64 = x.astype(np.float64)
    wd = G.decode_weights(dtype, w, rows, K).astype(np.float64)
    mags = R.mag_rows(dtype, w) if dtype in AFFINE else np.abs(wd)  # |d q| per element, + |m|
    err = np.abs(y - x64 @ wd.T)
    bound = 1e-5 * (np.abs(x64) @ mags.T) + 1e-7
    print(f"dtype {dtype} rows {rows} n {n} K {K} ks {ks}: worst err / bar {float((err / bound).max()):.3g}")
    assert np.all(err <= bound)
    assert np.array_equal(bits(y), bits(L.op_prompt_matmul_gq(x, w, dtype, rows, ks)))


@pytest.mark.parametrize("ks", [0, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_hot_probes_return_the_weights(dtype, ks):
    rows, K = G.N_CODES[dtype], 256  # every code at every block position, d and m through their extremes
    w = G.coded_weights(dtype, rows, K, False)
    want = np.float32(2.0) * G.decode_weights(dtype, w, rows, K).astype(np.float32)  # fmaf(d, q, m) in f32
    for c0 in range(0, K, BT):
        x = np.zeros((BT, K), np.float32)
        x[np.arange(BT), c0 + np.arange(BT)] = 2.0
        y = L.op_prompt_matmul_gq(x, w, dtype, rows, ks)
        assert np.array_equal(bits(y), bits(want[:, c0:c0 + BT].T + np.float32(0))), (dtype, ks, c0)


# ---- whole passes ---------------------------------------------------------------------------------
N_TOK, N_SCORED, CONTEXT = 100, 70, 256
FILES = {"q8_0": L.Q8_0, "q4_0": L.Q4_0, "q4_1": L.Q4_1, "q5_0": L.Q5_0, "q5_1": L.Q5_1}
_ORACLE = {}


def toks_of(vocab):
    return [1] + [3 + (i * 37) % (vocab - 3) for i in range(N_TOK - 1)]


def oracle_logits(xf, t, toks):
    """the token loop's logits at every position, once per file"""
    if t not in _ORACLE:
        om = R.oracle_from_xalm(xf, context=CONTEXT)
        lgs = []
        for pos, tok in enumerate(toks):
            om.forward(tok, pos)
            lgs.append(om.logits().copy())
        om.close()
        _ORACLE[t] = lgs
    return _ORACLE[t]


@pytest.mark.parametrize("option", [1, 0])
@pytest.mark.parametrize("t", list(FILES))
def test_passes_match_the_token_loop(t, option):
    xf = XalmFile(fixture_path(f"tiny_mistral_{t}.xalm"))
    gm = Model.from_xalm(xf, context=CONTEXT)
    gm.set_option(L.OPT_PREFILL_GQ, option)
    assert gm.get_option(L.OPT_PREFILL_GQ) == option
    toks = toks_of(gm.config.vocab_size)
    assert gm.prefill_route(N_TOK, 0) == (N_TOK, 2 if not option and FILES[t] in AFFINE else 1)
    lgs = oracle_logits(xf, t, toks)
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
        gm.set_option(L.OPT_PREFILL_GQ, option)
        st = InferenceState(gm.config)
        gm.prefill(toks_of(gm.config.vocab_size), 0, st)
        out.append(bits(st.logits()).copy())
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("bad", [2, -1])
def test_option_values(bad):
    gm = Model.from_xalm(XalmFile(fixture_path("tiny_mistral_q4_0.xalm")))
    gm.set_option(L.OPT_PREFILL_GQ, 1)
    with pytest.raises(L.XhError):
        gm.set_option(L.OPT_PREFILL_GQ, bad)
    assert gm.get_option(L.OPT_PREFILL_GQ) == 1
    gm.close()
