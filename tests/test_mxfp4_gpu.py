"""MXFP4 block weights on the device vs the CPU oracle.

The oracle does not decode the format, so it runs the reference forward over the rows dequantized
by tests/mxfp4_ref.py (pinned to the C quantizer / dequantizer by tests/test_mxfp4_cpu.py), as F32
tensors.  Bars: matvec |gpu - cpu| <= 2e-6 * mag + 1e-7 with mag = sum |w| |x| (tests/test_ops_gpu.py);
one-term products exactly; whole forward logits within bars.north; K/V rows within
2e-3 * max(1, max|ref|); synthetic forward within 1e-3 * max(1, max|ref|).
"""
import shutil

import numpy as np
import pytest

import bench
import mxfp4_ref as R
from bars import check_logp, north
from conftest import fixture_path
from oracle import oracle as O
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

FIXTURE = "tiny_mistral_mxfp4"
# one block per row; d below one wave's rows; d no multiple of the rows per workgroup; long rows
SHAPES = [(32, 8), (64, 32), (512, 96), (1536, 300), (4096, 64), (4096, 1025), (14336, 8)]
SCALES = [0, 1, 114, 127, 140, 254]


@pytest.mark.parametrize("n,d", SHAPES)
def test_matmul_against_the_oracle(n, d):
    rng = np.random.default_rng(n + 13 * d)
    wf = (rng.standard_normal((d, n)) * 0.05).astype(np.float32)
    x = rng.standard_normal(n).astype(np.float32)
    w = L.quantize_blocks(L.MXFP4, wf)
    got = L.op_matmul(x, w, L.MXFP4, n, d)
    cpu = O.matmul(x, R.dequantize(w), L.F32, n, d)
    mag = R.mag_rows(w) @ np.abs(x.astype(np.float64))
    err = np.abs(got - cpu)
    print("matvec", n, d, "max err / bar", float((err / (2e-6 * mag + 1e-7)).max()))
    assert np.all(err <= 2e-6 * mag + 1e-7), err.max()


@pytest.mark.parametrize("shift", range(6))
def test_every_code_under_extreme_scales_is_exact(shift):
    """(n, d) = (64, 64), packed by hand: row r holds code r % 16 in every position; the row's two
    blocks carry e = SCALES[shift] and SCALES[(shift + 3) % 6].  x is one-hot (positions 0, 15, 16, 31
    of either block), a power of two that keeps the one product a normal f32: the output is that
    product exactly.  A swapped nibble half is caught by test_nibble_halves below (here every
    position holds the same code); a lost sign, -0 read as a value, a flushed or mis-read scale here."""
    n, d = 64, 64
    es = (SCALES[shift], SCALES[(shift + 3) % 6])
    codes = np.broadcast_to((np.arange(d) % 16).astype(np.uint8)[:, None, None], (d, 2, 32))
    w = R.pack(np.broadcast_to(np.array(es)[None, :], (d, 2)), codes)
    assert np.array_equal(R.parts(w)[0].reshape(d, 2)[5], es)
    for blk in (0, 1):
        e = es[blk]
        xe = 100 if e <= 1 else -100 if e == 254 else 0
        for j in (0, 15, 16, 31):
            x = np.zeros(n, np.float32)
            x[32 * blk + j] = np.ldexp(np.float32(1), xe)
            got = L.op_matmul(x, w, L.MXFP4, n, d)
            want = np.ldexp(R.CODE_VALUES[np.arange(d) % 16].astype(np.float64), e - 127 + xe).astype(np.float32)
            assert np.isfinite(want).all() and (np.abs(want[want != 0]) >= np.finfo(np.float32).tiny).all()
            assert np.array_equal(got, want), (es, blk, j, got[:16], want[:16])


def test_nibble_halves_and_positions_are_exact():
    # every position of a block holds another code (element j: code (j + r) % 16), one-hot x walks all
    # 64 positions: a swapped nibble half or a permuted byte moves the output to another code's value
    n, d = 64, 64
    j = np.arange(32)
    codes = ((j[None, None, :] + np.arange(d)[:, None, None] + 5 * np.arange(2)[None, :, None]) % 16).astype(np.uint8)
    w = R.pack(np.full((d, 2), 127), codes)
    deq = R.dequantize(w)
    for pos in range(n):
        x = np.zeros(n, np.float32)
        x[pos] = 2.0
        assert np.array_equal(L.op_matmul(x, w, L.MXFP4, n, d), 2.0 * deq[:, pos]), pos


@pytest.mark.parametrize("fuse", [1, 0])
def test_forward_on_the_fixture(fuse):
    # every position's logits vs the oracle (the embedding gather included: embed is MXFP4), then the
    # prompt path and the device greedy loop; XH_OPT_FUSE_ATTN_WO 1 takes the two-launch route
    xf = XalmFile(fixture_path(FIXTURE + ".xalm"))
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
        assert err <= north(ref), (pos, err, north(ref))
    gm.reset()
    om.reset()
    gm.prefill(toks[:9], 0, st)
    for pos, tok in enumerate(toks[:9]):
        om.forward(tok, pos, L.OUTPUT_LOGITS if pos == 8 else L.HYDRATE_KV_CACHE)
    ref = om.logits()
    assert np.abs(st.logits() - ref).max() <= north(ref)
    out = gm.decode_greedy(9, 6)
    assert len(out) == 6
    pos, compared = 9, 0
    for t in out:
        lg = om.logits()
        if np.sort(lg)[-1] - np.sort(lg)[-2] > 1e-3:
            assert t == O.sample_argmax(lg), pos
            compared += 1
        om.forward(t, pos)
        pos += 1
    assert compared >= 5, compared
    gm.close()
    om.close()


DOWN = "l.0.mlp.down.weight"


def patched_copy(xf, tmp_path, name, new_bytes, tag):
    """A copy of the file with one tensor's bytes replaced (same size)."""
    path = str(tmp_path / f"{tag}.xalm")
    shutil.copyfile(xf.path, path)
    ti = xf.tensors[name]
    buf = np.ascontiguousarray(new_bytes, dtype=np.uint8).reshape(-1)
    assert buf.size == ti.size
    with open(path, "r+b") as f:
        f.seek(ti.offset)
        f.write(buf.tobytes())
    return path


@pytest.fixture(scope="module")
def prompt_models(tmp_path_factory):
    """The fixture, and a copy whose l.0.mlp.down values are 2^-20 times as large (the reference
    quantizer: the same codes under e - 20, below 114), so that one matrix of a model that otherwise
    takes the f16 image route has to take the f32-input route."""
    xf = XalmFile(fixture_path(FIXTURE + ".xalm"))
    rows = xf.tensors[DOWN].shape[0]
    w = np.ascontiguousarray(xf.raw(DOWN)).reshape(rows, -1)
    e = R.parts(w)[0]
    assert e.min() >= 114 and e.max() <= 140  # the fixture itself lies inside the image range
    low = R.lower_scales(w, 20)
    e2 = R.parts(low)[0]
    assert np.array_equal(e2, e - 20) and e2.max() < 114
    path = patched_copy(xf, tmp_path_factory.mktemp("mxfp4"), DOWN, low, "low_down")
    return {"image": xf, "wide": XalmFile(path)}


@pytest.mark.parametrize("which", ["image", "wide"])
@pytest.mark.parametrize("batched", [1, 3, 0])
def test_prompt_passes(prompt_models, which, batched):
    """100 tokens at context 256 vs the oracle's HYDRATE loop: last logits, every K/V row; then the
    perplexity path over 80 tokens (the lm_head GEMM decodes MXFP4 rows in registers)."""
    xf = prompt_models[which]
    n_tok, context = 100, 256
    gm = Model.from_xalm(xf, context=context)
    gm.set_option(L.OPT_PREFILL, batched)
    # the plan: every token batched; 64-token passes unless every layer matrix takes the f16 image
    nb, npass = gm.prefill_route(n_tok, 0)
    if batched == 0:
        assert nb == 0
    else:
        assert (nb, npass) == (n_tok, 1 if (batched == 1 and which == "image") else 2), (nb, npass)
    om = R.oracle_from_xalm(xf, context=context)
    toks = [1] + [3 + (i * 41) % (gm.config.vocab_size - 3) for i in range(n_tok - 1)]
    st = InferenceState(gm.config)
    gm.prefill(toks, 0, st)
    for pos, tok in enumerate(toks):
        om.forward(tok, pos, L.OUTPUT_LOGITS if pos == len(toks) - 1 else L.HYDRATE_KV_CACHE)
    ref = om.logits()
    err = float(np.abs(st.logits() - ref).max())
    assert err <= north(ref), (which, batched, err, north(ref))
    for layer in range(gm.config.n_layers):
        for kv in (0, 1):
            a = gm.kv_read(layer, kv, 0, len(toks)).view(np.float16).astype(np.float32)
            b = om.kv(layer, kv)[:len(toks)].view(np.float16).astype(np.float32)
            assert np.abs(a - b).max() <= 2e-3 * max(1.0, np.abs(b).max()), (layer, kv)
    gm.reset()
    om.reset()
    got = gm.token_probs(toks[:80])
    for pos in range(79):
        om.forward(toks[pos], pos)
        lg = om.logits()
        ref_p = O.sample_prob(lg, toks[pos + 1])
        if ref_p < 1e-30:
            assert got[pos] < 1e-30
            continue
        check_logp(float(abs(np.log(got[pos]) - np.log(ref_p))), lg, None, pos)
    gm.close()
    om.close()


@pytest.mark.parametrize("dim,hidden,layers", [(2048, 4096, 2), (4096, 2048, 1)])
def test_synthetic_blocks_forward(dim, hidden, layers):
    # device-generated blocks equal the host quantizer's over the same synthetic values: a byte that
    # differs moves a weight by a whole code step, far outside the bar
    dtype = L.MXFP4
    w = dict(dim=dim, hidden=hidden, layers=layers, heads=16, kv_heads=4, head_dim=128, vocab=1000, msl=256,
             theta=1e6, wdt=dtype, edt=dtype, cdt=dtype)
    c = bench.make_config(w)
    gm, om = Model(c), O.OracleModel(c)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
        gm.upload_synthetic(kind, layer, dt, seed, mean, std)
        rows, cols = bench.tensor_shape(c, kind)
        if dt == dtype:
            host = L.quantize_blocks(dt, O.synthetic(rows, cols, L.F32, seed, mean, std).reshape(rows, cols))
            om.set_tensor(kind, layer, L.F32, R.dequantize(host))
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


def test_upload_checks(tmp_path):
    xf = XalmFile(fixture_path(FIXTURE + ".xalm"))
    xq = XalmFile(fixture_path("tiny_mistral_q4_0.xalm"))
    gm = Model.from_xalm(xf)
    raw = np.ascontiguousarray(xf.raw("l.0.attn.q.weight"))
    with pytest.raises(L.XhError):  # one byte short of whole blocks
        gm.upload(L.WQ, 0, L.MXFP4, raw[:-1])
    gm.upload(L.WQ, 0, L.MXFP4, raw)
    with pytest.raises(L.XhError):  # q/k/v share one dtype
        gm.upload(L.WK, 0, L.Q4_0, np.ascontiguousarray(xq.raw("l.0.attn.k.weight")))
    bad = raw.copy()
    bad[17 * 3] = 255  # the scale byte of the fourth block: NaN
    with pytest.raises(L.XhError):
        gm.upload(L.WQ, 0, L.MXFP4, bad)
    with pytest.raises(L.XhError):
        L.op_matmul(np.zeros(32, np.float32), np.full((1, 17), 255, np.uint8), L.MXFP4, 32, 1)
    for pos in (0, 7, 1000):
        assert gm.active_bytes(pos) == active_bytes_ref(xf, gm.config, pos), pos
    gm.close()
    # the file route refuses the same tensor
    path = patched_copy(xf, tmp_path, "l.0.attn.q.weight", bad, "nan_scale")
    with pytest.raises(L.XhError):
        Model.from_xalm(XalmFile(path))


def test_file_loader_matches_host_upload():
    xf = XalmFile(fixture_path(FIXTURE + ".xalm"))
    outs = []
    for direct in (True, False):
        gm = Model.from_xalm(xf, direct=direct)
        st = InferenceState(gm.config)
        for pos, tok in enumerate([1, 5, 77, 200]):
            gm.forward(st, tok, pos)
        outs.append(st.logits().copy())
        gm.close()
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0], outs[1])


def test_cli_runs_on_the_fixture():
    # `xalm -d hip` opens the file (C++ reader, shape adaptation, xh_upload_file): completion tokens
    # follow the oracle's greedy choice where its top-two gap is clear; perplexity is finite
    import ctypes
    import os
    import re
    import subprocess

    from conftest import ROOT
    cli = os.path.join(ROOT, "xalm_amd", "bin", "xalm")
    path = fixture_path(FIXTURE + ".xalm")
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
