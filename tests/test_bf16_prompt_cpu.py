"""XH_OPT_PREFILL_BF16 without a device: the option id, the hook's export and NULL checks, and the
numpy statement of the three-piece bf16 split (gemm_bf16.h) that the GPU tests compare pieces against."""
import os
import re

import numpy as np
import pytest

from xalm_amd import _lib as L

E_INVALID = 1  # XH_E_INVALID


def bf16_rne(x):
    """f32 -> bf16 bits, round to nearest even (finite input)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_pieces(x):
    """b0 = bf16(x), b1 = bf16(x - b0), b2 = bf16((x - b0) - b1) in f32 arithmetic: uint16 [3, ...]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b0 = bf16_rne(x)
    r1 = x - bf16_val(b0)
    b1 = bf16_rne(r1)
    b2 = bf16_rne(r1 - bf16_val(b1))
    return np.stack([b0, b1, b2])


def test_option_id():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "xalm_hip.h")).read()
    ids = dict(re.findall(r"\b(XH_OPT_\w+) = (\d+)", re.search(r"enum xh_option \{(.*?)\};", hdr, re.S).group(1)))
    assert ids["XH_OPT_PREFILL_BF16"] == "10" and len(set(ids.values())) == len(ids)
    assert L.OPT_PREFILL_BF16 == 10


@pytest.mark.parametrize("null", [0, 1, 2])
def test_hook_rejects_null_without_a_device(null):
    y, x, w = np.zeros((1, 1), np.float32), np.zeros((1, 64), np.float32), np.zeros((1, 64), np.uint16)
    args = [L.ptr(a) for a in (y, x, w)]
    args[null] = None
    assert L.lib().xh_op_prompt_matmul_bf16(*args, 1, 64, 1, 0, None) == E_INVALID
    assert b"prompt_matmul_bf16" in L.lib().xh_last_error(None)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_three_pieces_are_exact_over_every_mantissa(sign):
    # every 24-bit significand at three exponents; each piece and each partial sum is exact in float64
    m = np.arange(1 << 23, dtype=np.uint32)
    for e in (27, 127, 227):
        x = ((e << 23) | m).view(np.float32) * np.float32(sign)
        p = bf16_val(bf16_pieces(x)).astype(np.float64)
        assert np.array_equal(p[0] + p[1] + p[2], x.astype(np.float64))
        assert np.all((p[2] == 0) | (np.abs(p[2]) >= np.abs(x) * 2.0 ** -24))
