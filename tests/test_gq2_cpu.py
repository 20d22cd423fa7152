"""Affine and 5-bit gguf blocks (Q4_1 / Q5_0 / Q5_1) on the host: the shared quantizer
(include/xalm_synth.h through xh_quantize_blocks) and the tests' numpy dequantizer
(tests/gq2_ref.py) against the reference's quants.py, bit for bit; the readers on the converter's
files; and the reference matvec over the dequantized rows inside the bar the GPU tests use.

tests/golden/gq2_golden.npz holds quants.py ``quantize`` bytes and ``dequantize`` floats of the
rows of make_gq2_fixtures.py (seeded rows, zeros, ties, a negative maximum, rounding boundaries,
f16-subnormal scales, constant blocks with d == 0, an all-positive row).
"""
import ctypes
import os

import numpy as np
import pytest

import gq2_ref as R
from conftest import ROOT, fixture_path
from oracle import oracle as O
from xalm_amd import _lib as L
from xalm_amd.xalm_file import XalmFile

G = np.load(fixture_path("gq2_golden.npz"))
G1 = np.load(fixture_path("gq_golden.npz"))
FIXTURES = {"tiny_mistral_q4_1": L.Q4_1, "tiny_mistral_q5_0": L.Q5_0, "tiny_mistral_q5_1": L.Q5_1}
BLOCK_BYTES = {L.Q4_1: 20, L.Q5_0: 22, L.Q5_1: 24}


@pytest.mark.parametrize("name", list(R.TYPES))
def test_quantize_blocks_matches_quants_py(name):
    got = L.quantize_blocks(R.TYPES[name], G["inputs"])
    assert got.shape == G[name].shape
    bad = np.argwhere(got != G[name])
    assert bad.size == 0, bad[:5]


@pytest.mark.parametrize("name,dtype", [("q8_0", L.Q8_0), ("q4_0", L.Q4_0)])
def test_quantize_blocks_is_the_old_quantizer(name, dtype):
    # one quantizer: the new entry point, the oracle's binding of the same header, quants.py
    for x in (G["inputs"], G1["inputs"]):
        assert np.array_equal(L.quantize_blocks(dtype, x), O.quantize_gq(dtype, x))
    assert np.array_equal(L.quantize_blocks(dtype, G1["inputs"]), G1[name])


def test_quantize_blocks_rejects_other_dtypes():
    with pytest.raises(ValueError):
        L.quantize_blocks(L.F16, np.zeros(32, np.float32))
    out = np.zeros(64, np.uint8)
    v = np.zeros(32, np.float32)
    assert L.lib().xh_quantize_blocks(L.F16, L.ptr(v), 1, L.ptr(out)) != 0
    assert L.lib().xh_quantize_blocks(L.Q5_0, None, 1, L.ptr(out)) != 0


@pytest.mark.parametrize("name", list(R.TYPES))
def test_reference_dequantizer_matches_quants_py(name):
    got = R.dequant(R.TYPES[name], G[name])
    assert got.dtype == np.float32 and got.shape == G[name + "_deq"].shape
    assert np.array_equal(got.view(np.uint32), G[name + "_deq"].view(np.uint32))


@pytest.mark.parametrize("name", list(FIXTURES))
def test_readers_on_converter_files(name):
    path = fixture_path(name + ".xalm")
    xf = XalmFile(path)
    cfg = xf.config()
    dt = FIXTURES[name]
    assert L.GQ_BLOCK_BYTES[dt] == BLOCK_BYTES[dt]
    q_dim, kv_dim = cfg.n_heads * cfg.head_dim, cfg.n_kv_heads * cfg.head_dim
    cols = {L.EMBED: cfg.dim, L.WCLS: cfg.dim, L.WQ: cfg.dim, L.WK: cfg.dim, L.WV: cfg.dim, L.WO: q_dim,
            L.W1: cfg.dim, L.W2: cfg.hidden_dim, L.W3: cfg.dim}
    rows = {L.EMBED: cfg.vocab_size, L.WCLS: cfg.vocab_size, L.WQ: q_dim, L.WK: kv_dim, L.WV: kv_dim, L.WO: cfg.dim,
            L.W1: cfg.hidden_dim, L.W2: cfg.dim, L.W3: cfg.hidden_dim}
    for kind, _, tname in R.model_tensors(xf):
        if kind in cols:
            assert xf.dtype(tname) == dt, tname
            rb = L.row_bytes(dt, cols[kind])
            assert rb == cols[kind] // 32 * BLOCK_BYTES[dt]
            assert tuple(xf.tensors[tname].shape) == (rows[kind], rb), tname
            assert xf.tensors[tname].size == rows[kind] * rb
        else:
            assert xf.dtype(tname) == L.BF16, tname  # norm vectors stay BF16
    # the C++ reader parses the same header (its type names included) to the same config
    lib = ctypes.CDLL(os.path.join(ROOT, "xalm_amd", "lib", "libxalm_host.so"))
    lib.xalm_read_config.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(L.XhConfig)]
    lib.xalm_host_last_error.restype = ctypes.c_char_p
    for context in (0, 16):
        c = L.XhConfig()
        assert lib.xalm_read_config(path.encode(), context, ctypes.byref(c)) == 0, lib.xalm_host_last_error()
        p = xf.config(context)
        for f, _ in L.XhConfig._fields_:
            assert getattr(c, f) == getattr(p, f), f


@pytest.mark.parametrize("name", list(R.TYPES))
def test_reference_matmul_is_inside_the_gpu_bar(name):
    # the oracle's F32 matvec over the dequantized golden rows vs the float64 dot product, under
    # the bar and magnitude of tests/test_gq2_gpu.py: the reference alone is inside it
    dt = R.TYPES[name]
    deq = R.dequant(dt, G[name])
    d, n = deq.shape
    x = np.random.default_rng(7).normal(0, 1, n).astype(np.float32)
    got = O.matmul(x, deq, L.F32, n, d)
    exact = deq.astype(np.float64) @ x.astype(np.float64)
    mag = R.mag_rows(dt, G[name]) @ np.abs(x.astype(np.float64))
    err = np.abs(got - exact)
    print(name, "max err / bar", float((err / (2e-6 * mag + 1e-7)).max()))
    assert np.all(err <= 2e-6 * mag + 1e-7)


@pytest.mark.parametrize("dtype", [L.Q4_1, L.Q5_1])
@pytest.mark.parametrize("n,d", R.POSITIVE_SHAPES)
def test_reference_is_inside_the_bar_on_the_positive_case(dtype, n, d):
    # the all-positive-weights case of tests/test_gq2_gpu.py: the reference's own error there
    w, x = R.positive_case(dtype, n, d)
    deq = R.dequant(dtype, w)
    exact = deq.astype(np.float64) @ x.astype(np.float64)
    mag = R.mag_rows(dtype, w) @ np.abs(x.astype(np.float64))
    err = np.abs(O.matmul(x, deq, L.F32, n, d) - exact)
    print(dtype, n, d, "max err / bar", float((err / (2e-6 * mag + 1e-7)).max()))
    assert np.all(err <= 0.25 * (2e-6 * mag + 1e-7))


def test_greedy_gap_rule_skips_at_most_one_step():
    # tests/test_gq2_gpu.py compares a greedy token only where the oracle's top-two gap exceeds
    # 1e-3; with its token stride at most 1 of the 6 steps per fixture may fall under that
    for name in FIXTURES:
        xf = XalmFile(fixture_path(name + ".xalm"))
        om = R.oracle_from_xalm(xf)
        toks = R.loop_tokens(xf.config().vocab_size)
        for pos, tok in enumerate(toks[:9]):
            om.forward(tok, pos)
        skipped = 0
        for pos in range(9, 15):
            lg = np.sort(om.logits())
            skipped += not (lg[-1] - lg[-2] > 1e-3)
            om.forward(O.sample_argmax(om.logits()), pos)
        om.close()
        assert skipped <= 1, (name, skipped)


def test_cli_cpu_device_still_throws_on_block_files():
    import subprocess
    cli = os.path.join(ROOT, "xalm_amd", "bin", "xalm")
    r = subprocess.run([cli, fixture_path("tiny_mistral_q5_1.xalm"), "-d", "cpu", "-n", "2"], capture_output=True, text=True)
    assert r.returncode != 0 and "oracle" in r.stderr
