"""MXFP4 on the host: xh_quantize_blocks / xh_dequantize_blocks against the numpy reference of
tests/mxfp4_ref.py (written from the format's definition), byte for byte and bit for bit; the
readers on the fixture; the launch shapes.

tests/golden/mxfp4_golden.npz holds the reference's bytes and floats for the rows of
make_mxfp4_fixtures.py (random blocks over 40 octaves, ties, saturation, zeros, f32 subnormals,
powers of two).
"""
import ctypes
import os

import numpy as np
import pytest

import mxfp4_ref as R
from conftest import ROOT, fixture_path
from xalm_amd import _lib as L
from xalm_amd.xalm_file import XalmFile

G = np.load(fixture_path("mxfp4_golden.npz"))
TIES = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def both(values):
    """The C quantizer's bytes, checked equal to the reference's; then both dequantizers."""
    got = L.quantize_blocks(L.MXFP4, values)
    ref = R.quantize(values)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, bad[:5]
    assert np.array_equal(bits(L.dequantize_blocks(L.MXFP4, got)), bits(R.dequantize(ref)))
    return got


def test_code_values_are_the_literal_table():
    table = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
    codes = np.arange(16, dtype=np.uint8).repeat(2).reshape(1, 1, 32)  # element j: code j // 2
    w = R.pack(np.full((1, 1), 127), codes)
    v = L.dequantize_blocks(L.MXFP4, w)[0]
    assert np.array_equal(bits(v[::2]), bits(np.array(table, np.float32)))  # the sign of -0 too
    assert np.array_equal(bits(v), bits(R.dequantize(w)[0]))
    assert L.MXFP4 == 25 and L.GQ_BLOCK_BYTES[L.MXFP4] == 17 and L.DTYPE_BY_NAME["MXFP4"] == L.MXFP4


def test_golden_file():
    assert G["values"].shape[0] >= 200
    got = L.quantize_blocks(L.MXFP4, G["values"])
    assert np.array_equal(got, G["bytes"])
    assert np.array_equal(R.quantize(G["values"]), G["bytes"])
    assert np.array_equal(bits(L.dequantize_blocks(L.MXFP4, G["bytes"])), bits(G["deq"]))
    assert np.array_equal(bits(R.dequantize(G["bytes"])), bits(G["deq"]))


def test_random_blocks_over_40_octaves():
    rng = np.random.default_rng(99)
    v = (rng.standard_normal((2000, 32)) * np.exp2(rng.uniform(-20, 20, (2000, 1)))).astype(np.float32)
    both(v)


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -40, 2.0 ** 60])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_ties_go_to_the_even_code(scale, sign):
    b = np.zeros((1, 32), np.float32)
    b[0, 0] = 6.0 * scale  # fixes E: amax * 2^-E = 6
    for k, t in enumerate(TIES):
        b[0, 1 + k] = t * scale * sign
    w = both(b)
    v = L.dequantize_blocks(L.MXFP4, w)[0]
    assert w[0, 0] == 127 + int(np.log2(scale))
    for k, t in enumerate(TIES):
        assert v[1 + k] == np.float32(TIES[t] * scale * sign), (t, v[1 + k])
    assert np.signbit(v[1]) == (sign < 0)  # 0.25 -> (-)0


def test_saturation_zero_subnormals_and_powers_of_two():
    # above 6 saturates at 6: amax 7.99 gives E = 0
    b = np.full((1, 32), 7.99, np.float32)
    b[0, 1] = -7.5
    b[0, 2] = 6.5
    w = both(b)
    v = L.dequantize_blocks(L.MXFP4, w)[0]
    assert w[0, 0] == 127 and v[0] == 6.0 and v[1] == -6.0 and v[2] == 6.0
    # all-zero blocks (also of -0): e = 0 and every code 0
    for z in (0.0, -0.0):
        w = both(np.full((1, 32), z, np.float32))
        assert not w.any()
    # f32 subnormals: E clamps at -127 (e = 0), the values come back as f32 subnormals (the largest
    # round up to 2 * 2^-127, the smallest normal)
    rng = np.random.default_rng(5)
    sub = rng.integers(1, 1 << 23, (64, 32)).astype(np.uint32).view(np.float32)
    w = both(sub)
    assert (w[:, 0] == 0).all()
    v = L.dequantize_blocks(L.MXFP4, w)
    assert (np.abs(v) <= np.finfo(np.float32).tiny).all() and (np.abs(v) < np.finfo(np.float32).tiny).any() and v.any()
    one = np.zeros((1, 32), np.float32)
    one[0, 0] = np.array([1], np.uint32).view(np.float32)[0]  # 2^-149: 0.25 * 2^-127, a tie to 0
    assert not both(one)[0, 1:].any()
    # amax at exact powers of two 2^p: E = p - 2, amax * 2^-E = 4 (code 6)
    for p in range(-149, 128):
        b = np.zeros((1, 32), np.float32)
        b[0, 7] = np.ldexp(np.float32(1), p)
        b[0, 8] = np.ldexp(np.float32(-0.75), p)
        w = both(b)
        E = max(p - 2, -127)
        assert w[0, 0] == E + 127, p
        if p >= -125:
            assert w[0, 1 + 7] & 15 == 6 and L.dequantize_blocks(L.MXFP4, w)[0, 7] == b[0, 7], p


def test_round_trip_of_every_emitted_block():
    # every block of the golden file is one the quantizer emitted: its values quantize to itself
    w = G["bytes"]
    assert np.array_equal(L.quantize_blocks(L.MXFP4, L.dequantize_blocks(L.MXFP4, w)), w)
    assert np.array_equal(R.quantize(R.dequantize(w)), w)


def test_invalid_inputs_are_rejected():
    out = np.zeros(17, np.uint8)
    for bad in (np.nan, np.inf, -np.inf):
        v = np.zeros(32, np.float32)
        v[11] = bad
        assert L.lib().xh_quantize_blocks(L.MXFP4, L.ptr(v), 1, L.ptr(out)) != 0
        with pytest.raises(L.XhError):
            L.quantize_blocks(L.MXFP4, v)
    w = R.pack(np.array([[127, 255]]), np.zeros((1, 2, 32), np.uint8))
    with pytest.raises(L.XhError):
        L.dequantize_blocks(L.MXFP4, w)
    with pytest.raises(ValueError):
        R.dequantize(w)
    f = np.zeros(64, np.float32)
    assert L.lib().xh_dequantize_blocks(L.F16, L.ptr(w), 1, L.ptr(f)) != 0
    assert L.lib().xh_dequantize_blocks(L.MXFP4, None, 1, L.ptr(f)) != 0
    assert L.lib().xh_dequantize_blocks(L.MXFP4, L.ptr(w), 1, None) != 0
    with pytest.raises(ValueError):
        L.dequantize_blocks(L.F16, w)


@pytest.mark.parametrize("dtype", [L.Q8_0, L.Q4_0, L.Q4_1, L.Q5_0, L.Q5_1])
def test_dequantize_covers_the_other_block_types(dtype):
    # the same values as the tests' numpy dequantizers of those types give
    import gq2_ref
    rng = np.random.default_rng(dtype)
    w = L.quantize_blocks(dtype, (rng.standard_normal((8, 256)) * 0.05).astype(np.float32))
    got = L.dequantize_blocks(dtype, w)
    if dtype in gq2_ref.TYPES.values():
        ref = gq2_ref.dequant(dtype, w)
    else:
        blk = w.reshape(-1, L.GQ_BLOCK_BYTES[dtype])
        d = blk[:, 0:2].copy().view(np.float16).astype(np.float32)
        q = blk[:, 2:].view(np.int8).astype(np.float32) if dtype == L.Q8_0 else \
            np.concatenate([blk[:, 2:] & 15, blk[:, 2:] >> 4], axis=1).astype(np.float32) - 8
        ref = (d * q).reshape(8, 256)
    assert np.array_equal(bits(got), bits(ref))


def test_symbols_are_exported():
    lib = L.lib()
    for name in ("xh_quantize_blocks", "xh_dequantize_blocks", "xh_gemv_shape", "xh_upload", "xh_upload_file",
                 "xh_upload_synthetic"):
        assert getattr(lib, name) is not None
    assert callable(L.dequantize_blocks)


def test_readers_agree_on_the_fixture():
    path = fixture_path("tiny_mistral_mxfp4.xalm")
    xf = XalmFile(path)
    src = XalmFile(fixture_path("tiny_mistral_f32.xalm"))
    cfg = xf.config()
    q_dim, kv_dim = cfg.n_heads * cfg.head_dim, cfg.n_kv_heads * cfg.head_dim
    cols = {L.EMBED: cfg.dim, L.WCLS: cfg.dim, L.WQ: cfg.dim, L.WK: cfg.dim, L.WV: cfg.dim, L.WO: q_dim,
            L.W1: cfg.dim, L.W2: cfg.hidden_dim, L.W3: cfg.dim}
    rows = {L.EMBED: cfg.vocab_size, L.WCLS: cfg.vocab_size, L.WQ: q_dim, L.WK: kv_dim, L.WV: kv_dim, L.WO: cfg.dim,
            L.W1: cfg.hidden_dim, L.W2: cfg.dim, L.W3: cfg.hidden_dim}
    for kind, _, tname in R.model_tensors(xf):
        if kind in cols:
            assert xf.tensors[tname].type == "MXFP4" and xf.dtype(tname) == L.MXFP4, tname
            rb = L.row_bytes(L.MXFP4, cols[kind])
            assert rb == cols[kind] // 32 * 17
            assert tuple(xf.tensors[tname].shape) == (rows[kind], rb), tname
            # the tool's bytes are the host quantizer's over the source tensor
            w = np.ascontiguousarray(src.raw(tname)).view(np.float32).reshape(rows[kind], cols[kind])
            assert np.array_equal(np.asarray(xf.raw(tname)).reshape(rows[kind], rb), R.quantize(w)), tname
        else:  # norm vectors are copied through
            assert xf.dtype(tname) == src.dtype(tname) and np.array_equal(xf.raw(tname), src.raw(tname)), tname
    for tname in src.tensors:
        if tname.startswith("tokenizer."):
            assert np.array_equal(xf.raw(tname), src.raw(tname)), tname
    assert os.path.getsize(path) < 100 * 1024
    lib = ctypes.CDLL(os.path.join(ROOT, "xalm_amd", "lib", "libxalm_host.so"))
    lib.xalm_read_config.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(L.XhConfig)]
    lib.xalm_host_last_error.restype = ctypes.c_char_p
    for context in (0, 16):
        c = L.XhConfig()
        assert lib.xalm_read_config(path.encode(), context, ctypes.byref(c)) == 0, lib.xalm_host_last_error()
        p = xf.config(context)
        for f, _ in L.XhConfig._fields_:
            assert getattr(c, f) == getattr(p, f), f


def test_fixture_greedy_gap_rule():
    # what tests/test_mxfp4_gpu.py relies on: at least 5 of the 6 greedy steps are compared
    xf = XalmFile(fixture_path("tiny_mistral_mxfp4.xalm"))
    om = R.oracle_from_xalm(xf)
    assert R.greedy_gap_count(om, R.loop_tokens(xf.config().vocab_size)) >= 5
    om.close()


@pytest.mark.parametrize("role", [L.ROLE_QKV, L.ROLE_GLU, L.ROLE_RESID, L.ROLE_LOGITS, L.ROLE_STORE])
@pytest.mark.parametrize("n", [32, 4096, 14336])
def test_gemv_shape_answers_for_mxfp4(role, n):
    s = L.gemv_shape(role, L.MXFP4, n)
    assert s >= 0 and (s & ~L.SHAPE_BIG_LDS) < len(L.SHAPE_NAMES), (role, n, s)
