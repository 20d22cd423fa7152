"""XH_OPT_PREFILL_SHORT without a device: the option id, the route id and the hook's argument checks."""
import os
import re

import numpy as np
import pytest

from xalm_amd import _lib as L

E_INVALID = 1  # XH_E_INVALID


def test_option_id():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "xalm_hip.h")).read()
    ids = dict(re.findall(r"\b(XH_OPT_\w+) = (\d+)", re.search(r"enum xh_option \{(.*?)\};", hdr, re.S).group(1)))
    assert ids["XH_OPT_PREFILL_SHORT"] == "13" and len(set(ids.values())) == len(ids)
    assert L.OPT_PREFILL_SHORT == 13
    assert L.ROUTE_SK not in (L.ROUTE_ROWMAJOR, L.ROUTE_F32, L.ROUTE_BF16, L.ROUTE_KQ, L.ROUTE_GQ)


# (null argument or None, dtype, rows, K, n, ks): every one refused before a device is touched
BAD = [(0, L.Q8_0, 1, 64, 1, 0), (1, L.Q4_K, 1, 256, 1, 0), (2, L.Q5_1, 1, 64, 1, 0),  # a NULL pointer
       (None, L.F16, 1, 64, 1, 0), (None, L.MXFP4, 1, 64, 1, 0),                       # another dtype
       (None, L.Q4_1, 1, 96, 1, 0), (None, L.Q6_K, 1, 128, 1, 0),                      # K not in whole 64s / 256s
       (None, L.Q8_0, 1, 64, 0, 0), (None, L.Q4_0, 1, 64, 65, 0), (None, L.Q5_0, 0, 64, 1, 0),  # n, rows
       (None, L.Q4_1, 1, 192, 1, 3), (None, L.Q8_0, 1, 192, 1, 2), (None, L.Q4_K, 1, 768, 1, 2),  # ks
       (None, L.Q5_0, 1, 2048, 1, 32), (None, L.Q5_1, 1, 64, 1, -1)]


@pytest.mark.parametrize("null,dtype,rows,K,n,ks", BAD)
def test_hook_rejects_bad_arguments_without_a_device(null, dtype, rows, K, n, ks):
    y, x, w = np.full((1, 1), 7.5, np.float32), np.zeros((1, 2048), np.float32), np.zeros((1, 64 * 34), np.uint8)
    args = [L.ptr(a) for a in (y, x, w)]
    if null is not None:
        args[null] = None
    assert L.lib().xh_op_prompt_matmul_sk(*args, dtype, rows, K, n, ks) == E_INVALID
    assert b"prompt_matmul_sk" in L.lib().xh_last_error(None) and y[0, 0] == 7.5
