"""XH_OPT_PREFILL_I8: the activation quantiser bit for bit, the int8 prompt GEMM (gemm_i8.h) through
xh_op_prompt_matmul_i8 against float64 of the defined operands, and whole passes against the oracle's token loop.
Tile: 256 weight rows x 128 tokens, 64-deep K steps (two blocks), slices a multiple of 64."""
import numpy as np
import pytest

import gq2_ref as Q
import i8_ref as R
import prompt_gemm_ref as G
from bars import north
from conftest import fixture_path
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

DTYPES = list(R.BIAS)
BR, BT = 256, 128


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_quantiser_bit_for_bit():
    rng, K = np.random.default_rng(5), 128
    x = np.zeros((4, K), np.float32)
    x[0, 40] = 3.0                                                         # all-zero blocks; a lone amax
    x[1, :32] = np.resize([127, .5, 1.5, 2.5, -.5, -1.5, -2.5, 3.5, 126.5, -126.5], 32)  # ties at .5 (inv = 1 / s_t)
    x[1, 32:] = rng.standard_normal(K - 32)
    x[2] = rng.standard_normal(K) * np.exp2(np.linspace(-20, 10, K))       # 2^-20 .. 2^10 in one row
    x[3] = rng.standard_normal(K)
    _y, codes, scales = L.op_prompt_matmul_i8(x, G.random_weights(rng, L.Q4_0, 3, K), L.Q4_0, 3, want_quant=True)
    hi, lo, _inv_s = G.split_exact(x)
    want_c, want_s = R.quantise(hi, lo)
    assert list(want_c[1, 1:7]) == [0, 2, 2, 0, -2, -2] and not want_c[0, :32].any()
    assert np.array_equal(codes, want_c) and np.array_equal(bits(scales), bits(want_s))


# (rows, n, K, ks): every edge of the tiling once, a few combinations
CASES = [(1, 1, 64, 0), (BR - 1, BT - 1, 128, 2), (BR, BT, 192, 1), (BR + 32, BT + 1, 128, 0), (BR + 32, 1, 192, 0),
         (1, BT + 1, 64, 1), (BR, BT - 1, 2048, 8)]


@pytest.mark.parametrize("rows,n,K,ks", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_against_float64(dtype, rows, n, K, ks):
    rng = np.random.default_rng(rows * 7 + n * 3 + K + dtype)
    w, x = G.random_weights(rng, dtype, rows, K), G.random_x(rng, n, K)
    y, codes, scales = L.op_prompt_matmul_i8(x, w, dtype, rows, ks, want_quant=True)
    hi, lo, inv_s = G.split_exact(x)
    y64, mag = R.gemm64(dtype, w, rows, K, codes, scales, inv_s)
    err, bound = np.abs(y - y64), R.bound(K, ks, mag)
    print(f"dtype {dtype} rows {rows} n {n} K {K} ks {ks}: worst err / bound {float((err / bound).max()):.3g}")
    assert np.all(err <= bound)
    assert np.array_equal(bits(y), bits(L.op_prompt_matmul_i8(x, w, dtype, rows, ks)))
    # the definition itself: half a code step per activation element off the unquantised product
    exact = G.halves_value(hi, lo, inv_s) @ G.decode_weights(dtype, w, rows, K).T
    assert np.all(np.abs(y - exact) <= R.definition_bound(dtype, w, rows, K, scales, inv_s) + bound)


# ---- whole passes ---------------------------------------------------------------------------------
N_TOK, CONTEXT = 100, 256
FILES = ["q8_0", "q4_0", "q4_1", "q5_0", "q5_1"]
# max |logit - oracle| / north(oracle) of the last position.  The int8 rounding is outside north()'s f32 premise, so
# the bar is twice the worst ratio measured over the five files (profiles/i8_prompt_err.txt); the route is
# bit-reproducible, so the margin covers fixture or compiler changes, not noise.
BAR = 2 * 6.4794  # q4_0, the worst of 6.3860 / 6.4794 / 4.6411 / 5.4213 / 6.1007


def prefill_logits(gm, toks):
    gm.reset()
    st = InferenceState(gm.config)
    gm.prefill(toks, 0, st)
    return st.logits().copy()


@pytest.mark.parametrize("t", FILES)
def test_passes_against_the_token_loop(t):
    xf = XalmFile(fixture_path(f"tiny_mistral_{t}.xalm"))
    gm = Model.from_xalm(xf, context=CONTEXT)
    toks = [1] + [3 + (i * 37) % (gm.config.vocab_size - 3) for i in range(N_TOK - 1)]
    before = prefill_logits(gm, toks)
    gm.set_option(L.OPT_PREFILL_I8, 1)
    assert gm.get_option(L.OPT_PREFILL_I8) == 1 and gm.prefill_route(N_TOK, 0) == (N_TOK, 1)
    got = prefill_logits(gm, toks)
    gm.set_option(L.OPT_PREFILL_I8, 0)
    assert np.array_equal(bits(prefill_logits(gm, toks)), bits(before))  # option 0: the bits of the other routes
    assert not np.array_equal(bits(got), bits(before))                   # option 1 took the route
    gm.close()
    om = Q.oracle_from_xalm(xf, context=CONTEXT)
    for pos, tok in enumerate(toks):
        om.forward(tok, pos)
    ref = om.logits().copy()
    om.close()
    ratio = float(np.abs(got - ref).max()) / north(ref)
    print(f"tiny_mistral_{t}: max |dlogit| / north = {ratio:.4g}")
    assert ratio <= BAR


def test_f16_model_ignores_the_option():
    from test_forward_gpu import synthetic_pair
    out = []
    for option in (0, 1):
        gm, _om = synthetic_pair(L.F16)
        gm.set_option(L.OPT_PREFILL_I8, option)
        st = InferenceState(gm.config)
        gm.prefill([1] + [3 + (i * 37) % (gm.config.vocab_size - 3) for i in range(N_TOK - 1)], 0, st)
        out.append(bits(st.logits()).copy())
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("bad", [2, -1])
def test_option_values(bad):
    gm = Model.from_xalm(XalmFile(fixture_path("tiny_mistral_q4_0.xalm")))
    gm.set_option(L.OPT_PREFILL_I8, 1)
    with pytest.raises(L.XhError):
        gm.set_option(L.OPT_PREFILL_I8, bad)
    assert gm.get_option(L.OPT_PREFILL_I8) == 1
    gm.close()
