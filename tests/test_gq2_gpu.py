"""Affine and 5-bit gguf blocks (Q4_1 / Q5_0 / Q5_1) on the device vs the CPU oracle.

The oracle does not decode these blocks, so it runs the reference forward over the rows
dequantized by tests/gq2_ref.py (pinned bit for bit to quants.py by tests/test_gq2_cpu.py), as
F32 tensors.  Bars: matvec |gpu - cpu| <= 2e-6 * mag + 1e-7 (tests/test_ops_gpu.py) with
mag = sum(|d q| + |m|) |x| (the affine kernel sums d * sum(q x) and m * sum(x) separately); whole
forward logits within bars.north = 1e-3 * max(1, max|logit|); K/V rows within 2e-3 * max(1, max|ref|).
"""
import numpy as np
import pytest

import bench
import gq2_ref as R
from bars import check_logp, north
from conftest import fixture_path
from oracle import oracle as O
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

GQ2 = [L.Q4_1, L.Q5_0, L.Q5_1]
FIXTURES = ["tiny_mistral_q4_1", "tiny_mistral_q5_0", "tiny_mistral_q5_1"]
SHAPES = [(64, 32), (512, 96), (4096, 64), (1536, 300), (14336, 8), (4096, 1025)]


def matvec_check(dtype, w, x, n, d):
    got = L.op_matmul(x, w, dtype, n, d)
    cpu = O.matmul(x, R.dequant(dtype, w), L.F32, n, d)
    mag = R.mag_rows(dtype, w) @ np.abs(x.astype(np.float64))
    err = np.abs(got - cpu)
    print("matvec", dtype, n, d, "max err / bar", float((err / (2e-6 * mag + 1e-7)).max()))
    assert np.all(err <= 2e-6 * mag + 1e-7), err.max()


@pytest.mark.parametrize("dtype", GQ2)
@pytest.mark.parametrize("n,d", SHAPES)
def test_matmul_blocks(dtype, n, d):
    rng = np.random.default_rng(n + 13 * d + dtype)
    wf = (rng.standard_normal((d, n)) * 0.05).astype(np.float32)
    x = rng.standard_normal(n).astype(np.float32)
    matvec_check(dtype, L.quantize_blocks(dtype, wf), x, n, d)


@pytest.mark.parametrize("dtype", [L.Q4_1, L.Q5_1])
@pytest.mark.parametrize("n,d", R.POSITIVE_SHAPES)
def test_matmul_all_positive_weights(dtype, n, d):
    # m dominates every block: a dropped m * sum(x) moves the result by about sqrt(n)
    w, x = R.positive_case(dtype, n, d)
    assert R.parts(dtype, w)[1].min() >= 1.0
    matvec_check(dtype, w, x, n, d)


@pytest.mark.parametrize("dtype", [L.Q5_0, L.Q5_1])
@pytest.mark.parametrize("n,d", [(512, 96), (4096, 64)])
def test_matmul_every_fifth_bit_set(dtype, n, d):
    # codes 16..31 only (packed by hand: no quantizer leaves the low half unused): a lost bit
    # plane moves every weight by 16 d
    rng = np.random.default_rng(n + 7 * dtype)
    q = rng.integers(16, 32, (d, n // 32, 32))
    dd = rng.uniform(0.002, 0.01, (d, n // 32))
    mm = rng.normal(0.0, 0.05, (d, n // 32))
    w = R.pack(dtype, dd, mm, q)
    x = rng.standard_normal(n).astype(np.float32)
    assert (R.parts(dtype, w)[2] >= (0 if dtype == L.Q5_0 else 16)).all()
    matvec_check(dtype, w, x, n, d)


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("fuse", [1, 0])
def test_forward_on_converter_blocks(name, fuse):
    # every position's logits vs the oracle, then the prompt path and the device greedy loop;
    # XH_OPT_FUSE_ATTN_WO 1 takes the two-launch route for block Wo
    xf = XalmFile(fixture_path(name + ".xalm"))
    gm = Model.from_xalm(xf)
    gm.set_option(L.OPT_FUSE_ATTN_WO, fuse)
    om = R.oracle_from_xalm(xf)
    st = InferenceState(gm.config)
    toks = R.loop_tokens(gm.config.vocab_size)
    assert len(toks) == 21
    for pos, tok in enumerate(toks):
        gm.forward(st, tok, pos)
        om.forward(tok, pos)
        ref = om.logits()
        err = float(np.abs(st.logits() - ref).max())
        assert err <= north(ref), (name, pos, err, north(ref))
    gm.reset()
    om.reset()
    gm.prefill(toks[:9], 0, st)
    for pos, tok in enumerate(toks[:9]):
        om.forward(tok, pos, L.OUTPUT_LOGITS if pos == 8 else L.HYDRATE_KV_CACHE)
    ref = om.logits()
    assert np.abs(st.logits() - ref).max() <= north(ref), name
    out = gm.decode_greedy(9, 6)
    assert len(out) == 6
    pos, compared = 9, 0
    for t in out:
        lg = om.logits()
        if np.sort(lg)[-1] - np.sort(lg)[-2] > 1e-3:
            assert t == O.sample_argmax(lg), (name, pos)
            compared += 1
        om.forward(t, pos)
        pos += 1
    assert compared >= 5, (name, compared)  # the gap rule may skip at most 1 of the 6 steps
    gm.close()
    om.close()


def prompt_check(name, batched, n_tok, context, kv_which):
    xf = XalmFile(fixture_path(name + ".xalm"))
    gm = Model.from_xalm(xf, context=context)
    gm.set_option(L.OPT_PREFILL, batched)
    om = R.oracle_from_xalm(xf, context=context)
    toks = [1] + [3 + (i * 41) % (gm.config.vocab_size - 3) for i in range(n_tok - 1)]
    st = InferenceState(gm.config)
    gm.prefill(toks, 0, st)
    for pos, tok in enumerate(toks):
        om.forward(tok, pos, L.OUTPUT_LOGITS if pos == len(toks) - 1 else L.HYDRATE_KV_CACHE)
    ref = om.logits()
    err = float(np.abs(st.logits() - ref).max())
    assert err <= north(ref), (name, batched, err, north(ref))
    for layer in range(gm.config.n_layers):
        for which in kv_which:
            a = gm.kv_read(layer, which, 0, len(toks)).view(np.float16).astype(np.float32)
            b = om.kv(layer, which)[:len(toks)].view(np.float16).astype(np.float32)
            assert np.abs(a - b).max() <= 2e-3 * max(1.0, np.abs(b).max()), (layer, which)
    gm.close()
    om.close()
    return xf, toks


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("batched", [1, 3, 0])
def test_block_prompt_passes(name, batched):
    """A 100-token prompt at context 256 (XH_OPT_PREFILL 1: Q5_0's exact f16 hi + lo images through
    gemm16.h, the affine types on the f32-input MFMA kernel decoding the blocks in registers; 3:
    that kernel for all; 0: the token loop) vs the oracle's HYDRATE loop: last logits, every K/V
    row; then the perplexity path over 80 tokens (lm_head GEMM over block rows)."""
    xf, toks = prompt_check(name, batched, 100, 256, (0, 1))
    gm2 = Model.from_xalm(xf, context=256)
    gm2.set_option(L.OPT_PREFILL, batched)
    om2 = R.oracle_from_xalm(xf, context=256)
    got = gm2.token_probs(toks[:80])
    for pos in range(79):
        om2.forward(toks[pos], pos)
        lg = om2.logits()
        ref = O.sample_prob(lg, toks[pos + 1])
        if ref < 1e-30:
            assert got[pos] < 1e-30
            continue
        check_logp(float(abs(np.log(got[pos]) - np.log(ref))), lg, None, pos)
    gm2.close()
    om2.close()


def test_q5_0_multi_pass_prefill():
    """2200 tokens at context 4096 = a full 2048-token gemm16.h pass over Q5_0's hi / lo images and
    a 152-token one attending over the first pass's K/V rows, vs the oracle's token loop."""
    prompt_check("tiny_mistral_q5_0", 1, 2200, 4096, (1,))


@pytest.mark.parametrize("dim,hidden,layers", [(2048, 4096, 2), (4096, 2048, 1)])
@pytest.mark.parametrize("dtype", GQ2)
def test_synthetic_blocks_forward(dtype, dim, hidden, layers):
    # device-generated blocks (synth_gq_kernel) equal the host quantizer's over the same synthetic
    # values: a byte that differs moves a weight by a whole code step, far outside the bar.  Dims
    # that take the long-row matvec shapes, and (dim 4096) the pipelined block shapes for qkv,
    # W1/W3 and lm_head (n = 4096) and Wo / W2 (n = 2048)
    w = dict(dim=dim, hidden=hidden, layers=layers, heads=16, kv_heads=4, head_dim=128, vocab=1000, msl=256,
             theta=1e6, wdt=dtype, edt=dtype, cdt=dtype)
    c = bench.make_config(w)
    gm, om = Model(c), O.OracleModel(c)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
        gm.upload_synthetic(kind, layer, dt, seed, mean, std)
        rows, cols = bench.tensor_shape(c, kind)
        if dt in GQ2:
            host = L.quantize_blocks(dt, O.synthetic(rows, cols, L.F32, seed, mean, std).reshape(rows, cols))
            om.set_tensor(kind, layer, L.F32, R.dequant(dt, host))
        else:
            om.set_tensor(kind, layer, dt, O.synthetic(rows, cols, dt, seed, mean, std))
    st = InferenceState(c)
    for pos, tok in enumerate([1, 17, 999, 3, 512]):
        gm.forward(st, tok, pos)
        om.forward(tok, pos)
        ref = om.logits()
        assert np.abs(st.logits() - ref).max() <= 1e-3 * max(1.0, float(np.abs(ref).max())), pos
    gm.close()
    om.close()


def active_bytes_ref(xf, cfg, pos):
    """Model::active_bytes (src/model.cpp:12-35) from the file's tensor byte sizes."""
    size = lambda name: xf.tensors[name].size
    g = xf.global_tensors(bool(cfg.tie_word_embeddings))
    total = size(g[L.EMBED]) // cfg.vocab_size + size(g[L.FINAL_NORM]) + size(g[L.WCLS])
    kv_len = min(cfg.max_seq_len, pos + 1)
    for layer in range(cfg.n_layers):
        total += sum(size(name) for name in xf.layer_tensors(layer).values())
        total += 2 * kv_len * cfg.n_kv_heads * cfg.head_dim * 2
    return total


def test_block_upload_checks():
    xf = XalmFile(fixture_path("tiny_mistral_q5_0.xalm"))
    xf1 = XalmFile(fixture_path("tiny_mistral_q5_1.xalm"))
    gm = Model.from_xalm(xf)
    raw = np.ascontiguousarray(xf.raw("l.0.attn.q.weight"))
    with pytest.raises(L.XhError):  # one byte short of whole blocks
        gm.upload(L.WQ, 0, L.Q5_0, raw[:-1])
    gm.upload(L.WQ, 0, L.Q5_0, raw)
    with pytest.raises(L.XhError):  # q/k/v share one dtype
        gm.upload(L.WK, 0, L.Q5_1, np.ascontiguousarray(xf1.raw("l.0.attn.k.weight")))
    for pos in (0, 7, 1000):
        assert gm.active_bytes(pos) == active_bytes_ref(xf, gm.config, pos), pos
    gm.close()
    for name in ("tiny_mistral_q4_1", "tiny_mistral_q5_1"):
        x = XalmFile(fixture_path(name + ".xalm"))
        m = Model.from_xalm(x)
        assert m.active_bytes(3) == active_bytes_ref(x, m.config, 3), name
        m.close()


def test_file_loader_matches_host_upload():
    # Model.from_xalm streams the file through xh_upload_file; the same fixture through xh_upload
    # from numpy gives the same logits, bit for bit
    xf = XalmFile(fixture_path("tiny_mistral_q5_1.xalm"))
    outs = []
    for direct in (True, False):
        gm = Model.from_xalm(xf, direct=direct)
        st = InferenceState(gm.config)
        for pos, tok in enumerate([1, 5, 77, 200]):
            gm.forward(st, tok, pos)
        outs.append(st.logits().copy())
        gm.close()
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("name", FIXTURES)
def test_cli_runs_on_converter_blocks(name):
    # `xalm -d hip` opens the file (C++ reader, shape adaptation, xh_upload_file): completion
    # tokens follow the oracle's greedy choice where its top-two gap is clear; perplexity agrees
    import ctypes
    import os
    import re
    import subprocess

    from conftest import ROOT
    cli = os.path.join(ROOT, "xalm_amd", "bin", "xalm")
    path = fixture_path(name + ".xalm")
    r = subprocess.run([cli, path, "-d", "hip", "-n", "10", "-i", "the answer is"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    ids = [int(v) for v in re.search(r"tokens: \[([0-9,]*)\]", r.stdout.decode("utf-8", errors="replace")).group(1).split(",")]
    xf = XalmFile(path)
    om = R.oracle_from_xalm(xf)
    host = ctypes.CDLL(os.path.join(ROOT, "xalm_amd", "lib", "libxalm_host.so"))
    out = (ctypes.c_int * 64)()
    n = ctypes.c_int(0)
    assert host.xalm_encode(path.encode(), b"the answer is", 1, out, 64, ctypes.byref(n)) == 0
    prompt = list(out[: n.value])
    assert ids[: len(prompt)] == prompt and len(ids) > len(prompt)
    for pos, tok in enumerate(ids[:-1]):
        om.forward(tok, pos)
        if pos >= len(prompt) - 1:
            lg = om.logits()
            top2 = np.sort(lg)[-2:]
            if top2[1] - top2[0] > 1e-3:
                assert ids[pos + 1] == O.sample_argmax(lg), pos
    om.close()
    text = "Q: What is the meaning of life? A: the answer is in the stars"
    r = subprocess.run([cli, path, "-d", "hip", "-m", "perplexity", "-i", text], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    m = re.search(r"^perplexity: (\S+)$", r.stdout.decode("utf-8", errors="replace"), re.M)
    assert m and np.isfinite(float(m.group(1))) and float(m.group(1)) > 1.0
