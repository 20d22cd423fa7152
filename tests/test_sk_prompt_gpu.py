"""XH_OPT_PREFILL_SHORT: the weight-streaming code GEMM for prompt passes of at most 64 tokens (gemm_sk.h) through
xh_op_prompt_matmul_sk against float64 and the dequantised weights, and whole passes against the oracle's token
loop.  Workgroup: 128 weight rows x all tokens in tiles of 16; 64-deep K steps; slices of whole 64s (the
K-quants: whole 256s), at most 16, the picker leaving at least 256 columns a slice."""
import numpy as np
import pytest

import gq2_ref as R
import kq_ref as KR
import prompt_gemm_ref as G
from bars import check_logp, north
from conftest import fixture_path
from oracle import oracle as O
from test_kq_gpu import every_code_matrix, kq_files, oracle_from_xalm  # noqa: F401 (kq_files: a fixture)
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

BLOCK = [L.Q8_0, L.Q4_0, L.Q4_1, L.Q5_0, L.Q5_1]
KQ = [L.Q4_K, L.Q6_K]
AFFINE = (L.Q4_1, L.Q5_1)
BR = 128


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# (rows, n, K of the block formats, K of the K-quants, ks): every edge of the tiling once.  K 64 / 256 the least;
# 384 / 1536 in two slices and 192 / 768 in one: three steps (super-blocks) a slice; 8 the most slices the picker
# takes at K 2048 (256 columns each), which ks 0 then takes for a single row tile
CASES = [(1, 1, 64, 256, 0), (BR - 1, 15, 384, 1536, 2), (BR, 16, 192, 768, 1), (BR + 1, 17, 128, 512, 0),
         (2 * BR + 40, 33, 192, 768, 0), (BR, 64, 2048, 2048, 8), (40, 64, 2048, 2048, 0)]


@pytest.mark.parametrize("rows,n,Kb,Kk,ks", CASES)
@pytest.mark.parametrize("dtype", BLOCK + KQ)
def test_gemm_against_float64(dtype, rows, n, Kb, Kk, ks):
    K = Kk if dtype in KQ else Kb
    rng = np.random.default_rng(rows * 7 + n * 3 + K + dtype)
    x = G.random_x(rng, n, K)
    if dtype in KQ:
        w = KR.random_blocks(dtype, rows * (K // 256), rng).reshape(rows, -1)
        wd, mags = KR.dequantize(dtype, w).astype(np.float64), KR.terms(dtype, w)
    else:
        w = G.random_weights(rng, dtype, rows, K)
        wd = G.decode_weights(dtype, w, rows, K).astype(np.float64)
        mags = R.mag_rows(dtype, w) if dtype in AFFINE else np.abs(wd)  # |d q| per element, + |m|
    y = L.op_prompt_matmul_sk(x, w, dtype, rows, ks)
    x64 = x.astype(np.float64)
    err = np.abs(y - x64 @ wd.T)
    bound = 1e-5 * (np.abs(x64) @ mags.T) + 1e-7
    print(f"dtype {dtype} rows {rows} n {n} K {K} ks {ks}: worst err / bar {float((err / bound).max()):.3g}")
    assert np.all(err <= bound)
    assert np.array_equal(bits(y), bits(L.op_prompt_matmul_sk(x, w, dtype, rows, ks)))


@pytest.mark.parametrize("ks", [0, 2])
@pytest.mark.parametrize("dtype", BLOCK + KQ)
def test_one_hot_probes_return_the_weights(dtype, ks):
    """every code at every block position under extreme scales: 2 x the dequantised weight bit for bit"""
    if dtype in KQ:
        rows, K = 64, 512
        w = every_code_matrix(dtype).reshape(rows, -1)
        want = 2.0 * KR.dequantize(dtype, w)
    else:
        rows, K = G.N_CODES[dtype], 256
        w = G.coded_weights(dtype, rows, K, False)
        want = np.float32(2.0) * G.decode_weights(dtype, w, rows, K).astype(np.float32)  # fmaf(d, q, m) in f32
    for c0 in range(0, K, 64):
        x = np.zeros((64, K), np.float32)
        x[np.arange(64), c0 + np.arange(64)] = 2.0
        y = L.op_prompt_matmul_sk(x, w, dtype, rows, ks)
        assert np.array_equal(bits(y), bits(want[:, c0:c0 + 64].T + np.float32(0))), (dtype, ks, c0)


# ---- whole passes ---------------------------------------------------------------------------------
N_TOK, N_SCORED, CONTEXT = 40, 30, 256
_ORACLE = {}


def toks_of(vocab, n=N_TOK):
    return [1] + [3 + (i * 37) % (vocab - 3) for i in range(n - 1)]


def oracle_logits(om_of, key, toks):
    """the token loop's logits at every position, once per file and length"""
    if key not in _ORACLE:
        om = om_of()
        lgs = []
        for pos, tok in enumerate(toks):
            om.forward(tok, pos)
            lgs.append(om.logits().copy())
        om.close()
        _ORACLE[key] = lgs
    return _ORACLE[key]


def check_passes(gm, lgs, toks, n_scored):
    route = gm.prefill_route(len(toks), 0)
    gm.set_option(L.OPT_PREFILL_SHORT, 1)
    assert gm.get_option(L.OPT_PREFILL_SHORT) == 1 and gm.prefill_route(len(toks), 0) == route
    st = InferenceState(gm.config)
    gm.prefill(toks, 0, st)
    err = float(np.abs(st.logits() - lgs[-1]).max())
    assert err <= north(lgs[-1]), (err, north(lgs[-1]))
    gm.reset()
    got = gm.token_probs(toks[:n_scored])
    for pos in range(n_scored - 1):
        ref_p = O.sample_prob(lgs[pos], toks[pos + 1])
        if ref_p < 1e-30:
            assert got[pos] < 1e-30
            continue
        check_logp(float(abs(np.log(got[pos]) - np.log(ref_p))), lgs[pos], None, pos)
    gm.close()


# the last: 100 tokens of Q4_1 with its long option off plan 64 + 36, both on the new route
@pytest.mark.parametrize("t,n", [("q8_0", N_TOK), ("q4_0", N_TOK), ("q4_1", N_TOK), ("q5_0", N_TOK), ("q5_1", N_TOK), ("q4_1", 100)])
def test_block_passes_match_the_token_loop(t, n):
    xf = XalmFile(fixture_path(f"tiny_mistral_{t}.xalm"))
    gm = Model.from_xalm(xf, context=CONTEXT)
    toks = toks_of(gm.config.vocab_size, n)
    if n > N_TOK:
        assert gm.get_option(L.OPT_PREFILL_GQ) == 0 and gm.prefill_route(n, 0) == (n, 2)
    lgs = oracle_logits(lambda: R.oracle_from_xalm(xf, context=CONTEXT), (t, n), toks)
    check_passes(gm, lgs, toks, N_SCORED if n == N_TOK else n - 10)


@pytest.mark.parametrize("t", ["q4_k_m", "q4_k", "q6_k"])
def test_kquant_passes_match_the_token_loop(kq_files, t):
    gm = Model.from_xalm(kq_files[t])
    toks = toks_of(gm.config.vocab_size)
    lgs = oracle_logits(lambda: oracle_from_xalm(kq_files[t]), (t, N_TOK), toks)
    check_passes(gm, lgs, toks, N_SCORED)


def test_f16_model_ignores_the_option():
    from test_forward_gpu import synthetic_pair
    out = []
    for option in (0, 1):
        gm, _om = synthetic_pair(L.F16)
        gm.set_option(L.OPT_PREFILL_SHORT, option)
        st = InferenceState(gm.config)
        gm.prefill(toks_of(gm.config.vocab_size), 0, st)
        out.append(bits(st.logits()).copy())
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("bad", [2, -1])
def test_option_values(bad):
    gm = Model.from_xalm(XalmFile(fixture_path("tiny_mistral_q4_0.xalm")))
    gm.set_option(L.OPT_PREFILL_SHORT, 1)
    with pytest.raises(L.XhError):
        gm.set_option(L.OPT_PREFILL_SHORT, bad)
    assert gm.get_option(L.OPT_PREFILL_SHORT) == 1
    gm.close()
