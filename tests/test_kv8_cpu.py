"""The fp8 (e4m3) KV ring's element on the host: xh_f8_e4m3_from_f32 against an independent float64
nearest-value search, and the reference's fp16 image of the codes.  No GPU."""
import numpy as np

from xalm_amd import _lib as L

import kv8_ref as R


def test_host_definition_matches_float64_search():
    x = R.quantizer_inputs()
    got = L.f8_e4m3_from_f32(x)
    want = np.concatenate([R.quantize_search(x[i:i + 8192]) for i in range(0, x.size, 8192)])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(x[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    # the named cases of the definition
    one = lambda v: int(L.f8_e4m3_from_f32(np.array([v], np.float32))[0])
    assert one(448.0) == 0x7E and one(449.0) == 0x7E and one(1e9) == 0x7E and one(-1e9) == 0xFE
    assert one(0.0) == 0x00 and one(-0.0) == 0x80
    assert one(2.0 ** -10) == 0x00 and one(-(2.0 ** -10)) == 0x80
    assert one(np.nextafter(np.float32(2.0 ** -10), np.float32(1))) == 0x01
    assert one(2.0 ** -9) == 0x01 and one(2.0 ** -6) == 0x08 and one(1.0) == 0x38
    assert not np.isin(got, [0x7F, 0xFF]).any()  # never the NaN code


def test_reference_image_is_exact_in_fp16():
    img = R.image16(R.FINITE).view(np.float16)
    assert R.FINITE.size == 254
    assert np.array_equal(img.astype(np.float64), R.VALUES[R.FINITE])
    # and the definition maps every code's value back to the code (the image of -0 is -0)
    assert np.array_equal(L.f8_e4m3_from_f32(img.astype(np.float32)), R.FINITE)


def test_symbols_are_exported():
    lib = L.lib()
    for n in ("xh_create_kv", "xh_kv_dtype", "xh_kv_write8", "xh_kv_read8", "xh_kv_sink_read", "xh_f8_e4m3_from_f32",
              "xh_op_kv_quantize", "xh_op_mha8"):
        assert hasattr(lib, n), n
