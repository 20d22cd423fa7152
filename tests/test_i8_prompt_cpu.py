"""XH_OPT_PREFILL_I8 without a device: the option id, the route id, the hook's argument checks, and the definition's
own error bound on the numpy reference."""
import os
import re

import numpy as np
import pytest

import i8_ref as R
import prompt_gemm_ref as G
from xalm_amd import _lib as L

E_INVALID = 1  # XH_E_INVALID


def test_option_and_route_ids():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "xalm_hip.h")).read()
    ids = dict(re.findall(r"\b(XH_OPT_\w+) = (\d+)", re.search(r"enum xh_option \{(.*?)\};", hdr, re.S).group(1)))
    assert ids["XH_OPT_PREFILL_I8"] == "14" and len(set(ids.values())) == len(ids)
    routes = (L.ROUTE_ROWMAJOR, L.ROUTE_F32, L.ROUTE_BF16, L.ROUTE_KQ, L.ROUTE_GQ, L.ROUTE_SK)
    assert L.OPT_PREFILL_I8 == 14 and L.ROUTE_I8 == -6 and L.ROUTE_I8 not in routes
    assert L.prompt_gemm_tile(L.ROUTE_I8) == 256


# (null argument or None, dtype, rows, K, n, ks): every one refused before a device is touched
BAD = [(0, L.Q8_0, 1, 64, 1, 0), (1, L.Q4_0, 1, 64, 1, 0), (2, L.Q5_1, 1, 64, 1, 0), (None, L.Q4_K, 1, 256, 1, 0),
       (None, L.MXFP4, 1, 64, 1, 0), (None, L.F16, 1, 64, 1, 0), (None, L.Q4_1, 1, 32, 1, 0), (None, L.Q5_0, 1, 96, 1, 0),
       (None, L.Q8_0, 1, 64, 0, 0), (None, L.Q8_0, 1, 64, 2049, 0), (None, L.Q4_0, 0, 64, 1, 0), (None, L.Q4_1, 1, 192, 1, 3),
       (None, L.Q5_0, 1, 1024, 1, 16), (None, L.Q5_1, 1, 64, 1, -1), (None, L.Q8_0, 1, 192, 1, 2)]


@pytest.mark.parametrize("null,dtype,rows,K,n,ks", BAD)
def test_hook_rejects_bad_arguments_without_a_device(null, dtype, rows, K, n, ks):
    y, x, w = np.full((1, 1), 7.5, np.float32), np.zeros((1, 1024), np.float32), np.zeros((1, 32 * 34), np.uint8)
    args = [L.ptr(a) for a in (y, x, w)]
    if null is not None:
        args[null] = None
    assert L.lib().xh_op_prompt_matmul_i8(*args, dtype, rows, K, n, ks, None, None) == E_INVALID
    assert b"prompt_matmul_i8" in L.lib().xh_last_error(None) and y[0, 0] == 7.5


@pytest.mark.parametrize("dtype", list(R.BIAS))
def test_definition_stays_within_half_a_code_step(dtype):
    """The reference alone: its product lies within the derived bound of the unquantised one."""
    rng, rows, n, K = np.random.default_rng(dtype), 40, 9, 128
    w, x = G.random_weights(rng, dtype, rows, K), G.random_x(rng, n, K)
    hi, lo, inv_s = G.split_exact(x)
    codes, scales = R.quantise(hi, lo)
    y64, mag = R.gemm64(dtype, w, rows, K, codes, scales, inv_s)
    exact = G.halves_value(hi, lo, inv_s) @ G.decode_weights(dtype, w, rows, K).T
    assert np.all(np.abs(y64 - exact) <= R.definition_bound(dtype, w, rows, K, scales, inv_s) + R.bound(K, 1, mag))
