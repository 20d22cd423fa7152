"""The fp8 form of the MFMA prompt attention without a device: the ABI surface (the op hook and the
option id), and the exactness its loader rests on: every finite e4m3 code has an f16 image that
holds its value exactly, so decoding a K/V tile to f16 loses nothing and the fp8 kernels can be
held to the fp16 kernels bit for bit (tests/test_kv8_prompt_attn_gpu.py)."""
import os
import re

import numpy as np

import kv8_ref as R
from conftest import ROOT
from test_host_cpu import declared_functions
from xalm_amd import _lib as L

HEADER = os.path.join(ROOT, "include", "xalm_hip.h")


def test_library_exports_the_hook():
    assert hasattr(L.lib(), "xh_op_prompt_attn8")
    assert "xh_op_prompt_attn8" in L._SIGNATURES


def test_header_declares_the_hook_and_the_option():
    assert "xh_op_prompt_attn8" in declared_functions(HEADER)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    enum = re.search(r"enum\s+xh_option\s*\{(.*?)\}", src, flags=re.S).group(1)
    ids = {k: int(v) for k, v in re.findall(r"(XH_OPT_\w+)\s*=\s*(\d+)", enum)}
    assert ids["XH_OPT_PREFILL_ATTN_KV8"] == 8 == L.OPT_PREFILL_ATTN_KV8
    assert len(set(ids.values())) == len(ids)  # no id is shared


def test_every_finite_code_has_an_exact_f16_image():
    codes = R.FINITE
    assert codes.size == 254 and 0x7F not in codes and 0xFF not in codes
    image = R.image16(codes).view(np.float16)
    assert np.isfinite(image).all()
    # exactly converted: the f16 holds the code's value (float64 definition), signed zeros included
    assert np.array_equal(image.astype(np.float64), R.image64(codes))
    assert np.array_equal(np.signbit(image), (codes & 0x80) != 0)
    # and no f16 subnormal is involved: the least e4m3 magnitude 2^-9 is a normal f16
    nz = image[image != 0]
    assert np.abs(nz).min() == 2.0 ** -9 and np.abs(nz).max() == 448.0
    # the round trip through the host definition of the ring's element
    assert np.array_equal(L.f8_e4m3_from_f32(image.astype(np.float32)), codes)
