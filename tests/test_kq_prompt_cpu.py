"""XH_OPT_PREFILL_KQ without a device: the option id, the hook's export and its argument checks."""
import os
import re

import numpy as np
import pytest

from xalm_amd import _lib as L

E_INVALID = 1  # XH_E_INVALID


def test_option_id():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "xalm_hip.h")).read()
    ids = dict(re.findall(r"\b(XH_OPT_\w+) = (\d+)", re.search(r"enum xh_option \{(.*?)\};", hdr, re.S).group(1)))
    assert ids["XH_OPT_PREFILL_KQ"] == "11" and len(set(ids.values())) == len(ids)
    assert L.OPT_PREFILL_KQ == 11 and L.ROUTE_KQ not in (L.ROUTE_ROWMAJOR, L.ROUTE_F32, L.ROUTE_BF16)


# (null argument or None, dtype, rows, K, n, ks): every one refused before a device is touched
BAD = [(0, L.Q4_K, 1, 256, 1, 0), (1, L.Q4_K, 1, 256, 1, 0), (2, L.Q6_K, 1, 256, 1, 0), (None, L.Q4_0, 1, 256, 1, 0),
       (None, L.Q4_K, 1, 128, 1, 0), (None, L.Q6_K, 1, 256, 0, 0), (None, L.Q6_K, 1, 256, 2049, 0),
       (None, L.Q4_K, 0, 256, 1, 0), (None, L.Q4_K, 1, 768, 1, 3), (None, L.Q4_K, 1, 256, 1, 16), (None, L.Q4_K, 1, 256, 1, -1)]


@pytest.mark.parametrize("null,dtype,rows,K,n,ks", BAD)
def test_hook_rejects_bad_arguments_without_a_device(null, dtype, rows, K, n, ks):
    y, x, w = np.zeros((1, 1), np.float32), np.zeros((1, 768), np.float32), np.zeros((1, 3 * 210), np.uint8)
    args = [L.ptr(a) for a in (y, x, w)]
    if null is not None:
        args[null] = None
    assert L.lib().xh_op_prompt_matmul_kq(*args, dtype, rows, K, n, ks) == E_INVALID
    assert b"prompt_matmul_kq" in L.lib().xh_last_error(None)
