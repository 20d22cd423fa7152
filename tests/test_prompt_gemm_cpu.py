"""The conditions the generators of tests/prompt_gemm_ref.py promise, checked with no device: the exact
cases are exact, the reference split keeps its bound, the forced K slicings divide as the pickers
require, and the hand-packed blocks decode to what they were packed from."""
import numpy as np
import pytest

from xalm_amd import _lib as L

import prompt_gemm_ref as R

NEW_EXPORTS = ("xh_op_prompt_matmul", "xh_op_prompt_weight_image", "xh_op_prompt_stage", "xh_prompt_gemm_tile")
ROUTES = [("f32", dt, -1) for dt in R.F32_ROUTE_DTYPES] + [("frag", dt, 8 if dt == L.F16 else 16) for dt in R.FRAG_DTYPES] + \
         [("rowmajor", dt, 0) for dt in R.ROWMAJOR_DTYPES]


def test_new_hooks_are_exported():
    for name in NEW_EXPORTS:
        assert hasattr(L.lib(), name), name


def test_tiles_come_from_the_library():
    assert L.prompt_gemm_tile(-1) % 32 == 0 and L.prompt_gemm_tile(8) % 32 == 0 and L.prompt_gemm_tile(0) % 32 == 0
    assert L.prompt_gemm_tile(8) == L.prompt_gemm_tile(16)


@pytest.mark.parametrize("dtype", [d for d in R.F32_ROUTE_DTYPES if d != L.Q8])  # XH_Q8 holds no integer but 0
def test_small_int_weights_decode_exactly(dtype):
    v =np.random.default_rng(1).integers(-2, 3, size=(5, 64))
    assert np.array_equal(R.decode_weights(dtype, R.small_int_weights(dtype, v), 5, 64), v.astype(np.float64))


@pytest.mark.parametrize("dtype", [d for d in R.F32_ROUTE_DTYPES if d != L.Q8])
@pytest.mark.parametrize("n", [1, 31, 33, 64])
def test_sparse_sums_are_exact(dtype, n):
    K = 16 * R.elems(dtype)
    x, w, v, units = R.sparse_case(np.random.default_rng(n + dtype), dtype, 40, K, n)
    assert np.all((x != 0).sum(axis=1) == 8)
    assert R.exact_terms_ok(x, v, units)
    # and a 22-bit value in every place would not be: the reason seven of the eight are shorter
    assert 8 * 2 * 2 ** 22 > 2 ** 24


@pytest.mark.parametrize("kind,dtype,route", ROUTES)
def test_probes_cover_what_they_claim(kind, dtype, route):
    chunk = 8 if route == 0 else R.elems(dtype) if route < 0 else route
    for K, ks in R.gemm_cases(kind, dtype):
        ks = max(ks, 1)
        kl = np.array(R.probe_ks(K, chunk, ks))
        assert set(kl // chunk) == set(range(K // chunk))                      # every chunk: both lane halves
        assert {0, K - 1} <= set(kl) and set(range(min(32, K))) <= set(kl % 32 if K >= 32 else kl)
        for s in range(ks):
            assert {s * (K // ks), (s + 1) * (K // ks) - 1} <= set(kl)
        x = R.probe_x(list(kl), K)
        assert np.all(x.sum(axis=1) == 1) and np.all((x != 0).sum(axis=1) == 1)
    rows = 3 * L.prompt_gemm_tile(route) + 33
    if dtype in R.ONE_BYTE or dtype in R.BLOCKS:
        K = R.gemm_cases(kind, dtype)[-1][0]
        w = R.coded_weights(dtype, rows, K, route == 0)
        wd = R.decode_weights(dtype, w, rows, K)
        assert np.all(np.isfinite(wd))
        if route == 0:
            assert np.all(np.abs(wd) <= 65504)
        cols = R.probe_ks(K, chunk, 1)
        if dtype in R.ONE_BYTE:
            want = {c for c in range(256) if dtype == L.Q8 or not R.f8_special(np.array(c), dtype)}
            assert want <= set(w[:, cols].reshape(-1).tolist())
        else:
            q = (np.arange(rows)[:, None] + 37 * np.array(cols)[None, :]) % R.N_CODES[dtype]
            for pos in range(32):
                at = q[:, np.array(cols) % 32 == pos]
                assert set(at.reshape(-1).tolist()) == set(range(R.N_CODES[dtype])), pos


def test_reference_split_bound():
    rng = np.random.default_rng(3)
    for n, K in [(33, 96), (64, 1032)]:
        x = R.random_x(rng, n, K)
        hi, lo, inv_s = R.split_exact(x)
        got = R.halves_value(hi, lo, inv_s)
        # the header's bound holds down to the f16 subnormal floor of lo (2^-38 of the row max)
        floor = np.abs(x).max(axis=1, keepdims=True).astype(np.float64) * 2.0 ** -38
        assert np.all(np.abs(got - x) <= 2.0 ** -22 * np.abs(x) + floor)
        h2, l2 = R.split16(x.astype(np.float64))
        assert np.array_equal(h2, hi) and np.array_equal(l2, lo)
    z = np.zeros((2, 32), np.float32)
    hi, lo, inv_s = R.split_exact(z)
    assert not hi.any() and not lo.any() and np.all(inv_s == 1.0)


@pytest.mark.parametrize("kind,dtype,route", ROUTES)
def test_forced_slicings_divide(kind, dtype, route):
    tile = L.prompt_gemm_tile(route)
    for K, ks in R.gemm_cases(kind, dtype):
        for rows in R.row_cases(tile):
            if ks:
                assert R.forced_ks_ok(route, dtype, rows, K, ks, tile), (K, ks, rows)
    assert not R.forced_ks_ok(route, dtype, 8, R.gemm_cases(kind, dtype)[0][0], 3, tile)


def test_float64_stages():
    x = np.array([[3.0, -4.0, 0.0, 0.0]])
    assert np.allclose(R.rmsnorm64(x, np.ones(4, np.float32), L.F32, 0.0), x / 2.5)
    assert np.allclose(R.glu64([0.0, 1.0], [2.0, 2.0], L.ACT_SILU), [0.0, 2.0 / (1.0 + np.exp(-1.0))])
    assert np.allclose(R.glu64([1.0], [1.0], L.ACT_GELU), [0.5 * (1 + np.tanh(0.797885 * 1.044715))])
