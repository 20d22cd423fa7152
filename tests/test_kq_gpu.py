"""The gguf K-quants (XH_Q4_K / XH_Q6_K) on the device.

References: tests/kq_ref.py (numpy, pinned to the reference's quants.py and to the C host code by
tests/test_kq_cpu.py) and the CPU oracle run over the dequantized rows as F32 tensors.
Bars: a one-term product exactly; matvec |gpu - f64| <= 2e-6 * sum (|d_eff q| + |m_eff|) |x| (Q6_K:
|d sc (q - 32)|), the block bar of DESIGN.md 4.8b; whole-model logits within bars.north; scored
tokens by bars.check_logp.

The Q4_K_M model (small_llama_f16.xalm through tools/xalm_requant.py) is made afresh per session: at
1.9 MB it is above the size of a committed file; tests/test_kq_cpu.py holds it to a recorded digest.
"""
import os
import sys

import numpy as np
import pytest

import bench
import kq_ref as R
import kq_stage_cases as KC
import stage_cases as SC
import stage_ref as SR
import test_stages_gpu as TS
from bars import check_logp, north
from kv8_ref import Kv8Ref, image64, ulp8
from conftest import ROOT, fixture_path
from oracle import oracle as O
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

sys.path.insert(0, os.path.join(ROOT, "tools"))
import xalm_requant  # noqa: E402

pytestmark = pytest.mark.gpu

DTS = {"q4_k": L.Q4_K, "q6_k": L.Q6_K}


# ---- one-hot exactness ------------------------------------------------------------------------
def every_code_matrix(dtype):
    """[rows][512 columns as bytes]: every code at every kind of position under the extreme
    sub-block fields.  Q4_K: row r, sub-block j: sc = F[(r + j) % 4], mn = F[(r + j + 1) % 4] with
    F = {0, 1, 31, 63}; element e holds code (e + r) % 16.  Q6_K: group g has scale
    S[(r + g) % 5], S = {-128, -1, 0, 1, 127}; element e holds code (e + 3 r) % 64."""
    rows, nsb = 64, 2
    blk = np.zeros((rows, nsb, R.BYTES[dtype]), np.uint8)
    e = np.arange(256)
    for r in range(rows):
        for b in range(nsb):
            o = blk[r, b]
            if dtype == L.Q4_K:
                F = [0, 1, 31, 63]
                sc = [F[(r + j + b) % 4] for j in range(8)]
                mn = [F[(r + j + b + 1) % 4] for j in range(8)]
                o[0:2] = np.array([0.0123], np.float16).view(np.uint8)
                o[2:4] = np.array([0.0457], np.float16).view(np.uint8)
                for j in range(4):
                    o[4 + j] = sc[j] | ((sc[j + 4] >> 4) << 6)
                    o[8 + j] = mn[j] | ((mn[j + 4] >> 4) << 6)
                    o[12 + j] = (sc[j + 4] & 15) | ((mn[j + 4] & 15) << 4)
                q = ((e + r + 5 * b) % 16).reshape(4, 2, 32)
                o[16:144] = (q[:, 0] | (q[:, 1] << 4)).reshape(128)
            else:
                S = [-128, -1, 0, 1, 127]
                o[192:208] = np.array([S[(r + g + b) % 5] for g in range(16)], np.int8).view(np.uint8)
                o[208:210] = np.array([-0.0371], np.float16).view(np.uint8)
                q = ((e + 3 * r + 7 * b) % 64).reshape(2, 4, 32)
                for h in range(2):
                    o[64 * h:64 * h + 32] = (q[h, 0] & 15) | ((q[h, 2] & 15) << 4)
                    o[64 * h + 32:64 * h + 64] = (q[h, 1] & 15) | ((q[h, 3] & 15) << 4)
                    o[128 + 32 * h:160 + 32 * h] = (q[h, 0] >> 4) | ((q[h, 1] >> 4) << 2) | ((q[h, 2] >> 4) << 4) | ((q[h, 3] >> 4) << 6)
    return np.ascontiguousarray(blk.reshape(rows, -1))


@pytest.mark.parametrize("name", sorted(DTS))
def test_one_hot_products_are_exact(name):
    dt = DTS[name]
    w = every_code_matrix(dt)
    deq = R.dequantize(dt, w)
    n, d = deq.shape[1], deq.shape[0]
    if dt == L.Q4_K:
        _, _, sc, mn, q = R.q4k_fields(w.reshape(-1, 144))
        assert set(np.unique(sc)) == {0, 1, 31, 63} == set(np.unique(mn)) and set(np.unique(q)) == set(range(16))
    else:
        _, sc, q = R.q6k_fields(w.reshape(-1, 210))
        assert set(np.unique(sc)) == {-128, -1, 0, 1, 127} and set(np.unique(q)) == set(range(64))
    for pos in range(n):
        x = np.zeros(n, np.float32)
        x[pos] = 2.0
        got = L.op_matmul(x, w, dt, n, d)
        assert np.array_equal(got, 2.0 * deq[:, pos]), (pos, got[:8], deq[:8, pos])


@pytest.mark.parametrize("name", sorted(DTS))
def test_embedding_gather_is_exact(name):
    """The one-hot matrix as the embedding of a 1-layer model whose layer adds nothing (Wo and W2
    zero) and whose final norm weight is 1: x after the layer is the gathered row, and the logits
    against a one-hot-row F32 lm_head return rmsnorm(row)[c]; compared with the same model holding the
    dequantized rows as an F32 embedding: bit-identical logits."""
    dt = DTS[name]
    w = every_code_matrix(dt)
    deq = R.dequantize(dt, w)
    vocab, dim = deq.shape
    c = bench.make_config(dict(dim=dim, hidden=256, layers=1, heads=4, kv_heads=4, head_dim=128, vocab=vocab, msl=16,
                               theta=1e4, wdt=L.F32, edt=dt, cdt=L.F32))
    outs = []
    for edt, emb in ((dt, w), (L.F32, deq)):
        gm = Model(c)
        z = lambda r, k: np.zeros((r, k), np.float32)
        gm.upload(L.EMBED, 0, edt, emb)
        cls = np.zeros((vocab, dim), np.float32)
        cls[np.arange(vocab), (np.arange(vocab) * 7) % dim] = 1.0
        gm.upload(L.WCLS, 0, L.F32, cls)
        gm.upload(L.FINAL_NORM, 0, L.F32, np.ones(dim, np.float32))
        for kind, shp in ((L.WQ, (512, dim)), (L.WK, (512, dim)), (L.WV, (512, dim)), (L.WO, (dim, 512)),
                          (L.W1, (256, dim)), (L.W3, (256, dim)), (L.W2, (dim, 256))):
            gm.upload(kind, 0, L.F32, z(*shp))
        gm.upload(L.ATTN_NORM, 0, L.F32, np.ones(dim, np.float32))
        gm.upload(L.FFN_NORM, 0, L.F32, np.ones(dim, np.float32))
        st = InferenceState(c)
        rows = []
        for pos, tok in enumerate(range(0, vocab, 5)):
            gm.forward(st, tok, pos % 16)
            rows.append(st.logits().copy())
        gm.close()
        outs.append(np.stack(rows))
    assert np.isfinite(outs[1]).all() and np.abs(outs[1]).max() > 0
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


# ---- matvec parity ----------------------------------------------------------------------------
# columns: one, two, three (odd) super-blocks, the GQL steps (2048, 6144) and the GQ step (4096);
# rows: one, below a wave's pair, one workgroup's worth, more than one round with an odd tail
MATVEC = [(256, 1), (256, 3), (512, 64), (768, 3), (768, 1000), (2048, 64), (4096, 1), (4096, 1000), (6144, 3)]


def test_matvec_cases_reach_every_shape_of_the_role():
    # op_matmul is (PRO_PLAIN, EPI_STORE): the dispatch can take GQ, GQL and the staged LONG shape
    for dt in DTS.values():
        got = {L.gemv_shape(L.ROLE_STORE, dt, n) & ~L.SHAPE_BIG_LDS for n, _ in MATVEC}
        names = {L.SHAPE_NAMES[s] for s in got}
        assert names == {"GQ", "GQL", "Long"}, names


@pytest.mark.parametrize("n,d", MATVEC)
@pytest.mark.parametrize("name", sorted(DTS))
def test_matvec_against_float64(name, n, d):
    dt = DTS[name]
    rng = np.random.default_rng(n + 17 * d + dt)
    w = R.random_blocks(dt, d * (n // 256), rng, scale_exp=(-10, -4)).reshape(d, -1)
    x = rng.standard_normal(n).astype(np.float32)
    got = L.op_matmul(x, w, dt, n, d)
    ref = R.dequantize(dt, w).astype(np.float64) @ x.astype(np.float64)
    bar = 2e-6 * (R.terms(dt, w) @ np.abs(x.astype(np.float64)))
    err = np.abs(got - ref)
    print("matvec", name, n, d, "max err / bar", float((err / bar).max()))
    assert np.all(err <= bar), float((err / bar).max())


def test_rejections_on_the_device_routes():
    with pytest.raises(L.XhError):  # 288 columns: no whole super-block
        L.op_matmul(np.zeros(288, np.float32), np.zeros((1, 162), np.uint8), L.Q4_K, 288, 1)
    c = bench.make_config(dict(dim=288, hidden=288, layers=1, heads=9, kv_heads=9, head_dim=32, vocab=8, msl=16,
                               theta=1e4, wdt=L.F32, edt=L.F32, cdt=L.F32))
    gm = Model(c)
    with pytest.raises(L.XhError):
        gm.upload(L.W2, 0, L.Q6_K, np.zeros((288, 288 // 32 * 26), np.uint8))
    with pytest.raises(L.XhError):
        gm.upload_synthetic(L.W2, 0, L.Q4_K, 1, 0.0, 0.02)
    with pytest.raises(L.XhError):  # a norm is no matrix
        gm.upload(L.ATTN_NORM, 0, L.Q4_K, np.zeros(162, np.uint8))
    gm.close()


# ---- every role at every launch shape, stage by stage ---------------------------------------------
def qkv8_stage(c, wdt, W):
    """The fp8-KV qkv writer (EPI_QKV8) of the case on an fp8 ring: {stage: worst err / bar}.  q at
    the stage bar of tests/stage_ref.py; the K/V codes of the new slot by the rule of tests/kv8_ref.py,
    |image(code) - clamp(ref)| <= ulp8(ref) / 2 + the stage's f32 bar."""
    gm = Model(SC.config(c), kv_dtype=L.F8_E4M3)
    for kind, dt, seed, mean, std in SR.tensor_specs(c, wdt):
        gm.upload_synthetic(kind, 0, dt, seed, mean, std)
    for which in (0, 1):
        gm.kv_fill_synthetic(0, which, 0, SC.HIST, SR.KV_SEED[which], 1.0)
    gm.forward(None, SC.TOKEN, SC.HIST, L.HYDRATE_KV_CACHE)
    q = gm.debug_read(L.READ_Q)
    codes = {"k8": gm.kv_read8(0, 0, SC.HIST, 1)[0], "v8": gm.kv_read8(0, 1, SC.HIST, 1)[0]}
    gm.close()
    edt, emb = W[L.EMBED]
    x0 = SR.decode64(edt, emb[SC.TOKEN:SC.TOKEN + 1], c.dim)[0][0]
    xn = SR.rmsnorm64(x0, SR.norm64(*W[L.ATTN_NORM]), 1e-5)
    cs = SR.rope_cs(c, SC.HIST)
    ratio = {}
    for name, kind in (("q8", L.WQ), ("k8", L.WK), ("v8", L.WV)):
        y, b = SR.matvec(*SR.decode64(W[kind][0], W[kind][1], c.dim), xn)
        if name != "v8":
            y, b = SR.rope_bar(c, y, b, cs)
        if name == "q8":
            ratio[name] = float(np.max(np.abs(q - y) / b))
        else:
            ref = np.clip(y, -448.0, 448.0)
            ratio[name] = float(np.max(np.abs(image64(codes[name]) - ref) / (ulp8(ref) / 2 + b)))
    return ratio


@pytest.mark.parametrize("c,wdt", KC.all_cases(), ids=[SC.case_id(c, d) for c, d in KC.all_cases()])
def test_stages_at_every_shape(c, wdt, monkeypatch):
    """tests/kq_stage_cases.py: one decode step of a one-layer model, every stage (QKV, attention +
    Wo, GLU, W2, LOGITS, the greedy argmax) against the float64 stages of tests/stage_ref.py at the
    block bar 2e-6 sum (|d_eff q| + |m_eff|) |x| + 1e-7, then the QKV8 writer on an fp8 ring."""
    KC.install(monkeypatch)
    W = SR.host_weights(c, wdt)
    o, gm, st = TS.observe(c, wdt, W)
    gm.close()
    ratio = SR.check_stages(c, wdt, W, o)
    ratio.update(qkv8_stage(c, wdt, W))
    ids = TS.shape_ids(c, wdt)
    ids.update({"q8": (5, c.dim), "k8": (5, c.dim), "v8": (5, c.dim)})
    report = {s: (SC.DT_NAME[wdt], ids[s][1], L.SHAPE_NAMES[L.gemv_shape(ids[s][0], wdt, ids[s][1]) & ~L.SHAPE_BIG_LDS], round(r, 4))
              for s, r in ratio.items()}
    print("stage: (dtype, n, shape, worst err / bar)", report)
    bad = {s: v for s, v in report.items() if not ratio[s] <= 1.0}
    assert not bad, bad


# ---- whole model --------------------------------------------------------------------------------
def oracle_from_xalm(xf, context=0):
    cfg = xf.config(context)
    om = O.OracleModel(cfg)
    from mxfp4_ref import model_tensors
    for kind, layer, name in model_tensors(xf):
        dt = xf.dtype(name)
        raw = np.ascontiguousarray(xf.raw(name))
        if dt in R.BYTES:
            om.set_tensor(kind, layer, L.F32, R.dequantize(dt, raw.reshape(xf.tensors[name].shape[0], -1)))
        else:
            om.set_tensor(kind, layer, dt, raw)
    return om


@pytest.fixture(scope="module")
def kq_files(tmp_path_factory):
    td = tmp_path_factory.mktemp("kq")
    out = {}
    for t in ("q4_k_m", "q4_k", "q6_k"):
        path = str(td / f"small_llama_{t}.xalm")
        xalm_requant.requant(fixture_path("small_llama_f16.xalm"), path, t)
        out[t] = XalmFile(path)
    return out


class DeqFile:
    """The file with its K-quant tensors presented as F32 (for references that decode by dtype)"""

    def __init__(self, xf):
        self.xf = xf
        self.config, self.global_tensors, self.layer_tensors = xf.config, xf.global_tensors, xf.layer_tensors

    def dtype(self, name):
        return L.F32 if self.xf.dtype(name) in R.BYTES else self.xf.dtype(name)

    def raw(self, name):
        dt, raw = self.xf.dtype(name), np.ascontiguousarray(self.xf.raw(name))
        if dt not in R.BYTES:
            return raw
        return R.dequantize(dt, raw.reshape(self.xf.tensors[name].shape[0], -1)).reshape(-1).view(np.uint8)


def loop_tokens(vocab, n=24):
    return [1] + [3 + (i * 37) % (vocab - 3) for i in range(n - 1)]


@pytest.fixture(scope="module")
def oracle_loops(kq_files):
    """Per file: the oracle's logits of the 24-step loop, computed once and shared"""
    out = {}
    for t, xf in kq_files.items():
        om = oracle_from_xalm(xf)
        toks = loop_tokens(xf.config().vocab_size)
        rows = []
        for pos, tok in enumerate(toks):
            om.forward(tok, pos)
            rows.append(om.logits().copy())
        om.close()
        out[t] = (toks, np.stack(rows))
    return out


@pytest.mark.parametrize("kv", ["f16", "f8"])
@pytest.mark.parametrize("t", ["q4_k_m", "q4_k", "q6_k"])
def test_forward_and_greedy(kq_files, oracle_loops, t, kv):
    xf = kq_files[t]
    toks, ref = oracle_loops[t]
    gm = Model.from_xalm(xf, kv_dtype=L.F8_E4M3 if kv == "f8" else L.F16)
    st = InferenceState(gm.config)
    if kv == "f16":
        for pos, tok in enumerate(toks):
            gm.forward(st, tok, pos)
            err = float(np.abs(st.logits() - ref[pos]).max())
            assert err <= north(ref[pos]), (pos, err, north(ref[pos]))
    if kv == "f8":
        # the fp8 ring's forward check (tests/test_kv8_gpu.py): its verify-then-adopt reference over
        # the dequantized rows, within bars.north at every step
        ref8 = Kv8Ref(DeqFile(xf))
        for pos, tok in enumerate(toks):
            gm.forward(st, tok, pos)
            want = ref8.step(tok, pos, gm)
            err = float(np.abs(st.logits() - want).max())
            assert err <= north(want), (pos, err, north(want))
        assert ref8.worst <= 1.0
    # the device greedy loop, graphs on and off, equals the forward argmax chain
    chains = []
    for graphs in (1, 0):
        gm.reset()
        gm.set_graphs(bool(graphs))
        for pos, tok in enumerate(toks[:8]):
            gm.forward(st, tok, pos)
        chains.append(list(gm.decode_greedy(8, 6)))
    gm.reset()
    gm.set_graphs(True)
    for pos, tok in enumerate(toks[:8]):
        gm.forward(st, tok, pos)
    want, pos = [], 8
    for _ in range(6):
        tok = int(O.sample_argmax(st.logits()))
        want.append(tok)
        gm.forward(st, tok, pos)
        pos += 1
    assert chains[0] == want and chains[1] == want, (chains, want)
    gm.close()


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("t", ["q4_k_m", "q4_k", "q6_k"])
def test_prefill_and_score(kq_files, t, mode):
    xf = kq_files[t]
    gm = Model.from_xalm(xf)
    gm.set_option(L.OPT_PREFILL, mode)
    vocab = gm.config.vocab_size
    toks = [1] + [3 + (i * 41) % (vocab - 3) for i in range(39)]
    # the plan equals Q4_1's of the same shapes
    g41 = Model(gm.config)
    w = dict(dim=gm.config.dim, hidden=gm.config.hidden_dim, layers=gm.config.n_layers, heads=gm.config.n_heads,
             kv_heads=gm.config.n_kv_heads, head_dim=gm.config.head_dim, vocab=vocab, msl=gm.config.max_seq_len,
             theta=1e4, wdt=L.Q4_1, edt=L.Q4_1, cdt=L.Q4_1)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
        g41.upload_synthetic(kind, layer, dt, seed, mean, std)
    g41.set_option(L.OPT_PREFILL, mode)
    assert gm.prefill_route(len(toks), 0) == g41.prefill_route(len(toks), 0)
    g41.close()
    om = oracle_from_xalm(xf)
    st = InferenceState(gm.config)
    gm.prefill(toks, 0, st)
    lgs = []
    for pos, tok in enumerate(toks):
        om.forward(tok, pos)
        lgs.append(om.logits().copy())
    err = float(np.abs(st.logits() - lgs[-1]).max())
    assert err <= north(lgs[-1]), (t, mode, err, north(lgs[-1]))
    gm.reset()
    got = gm.token_probs(toks)
    for pos in range(len(toks) - 1):
        ref_p = O.sample_prob(lgs[pos], toks[pos + 1])
        if ref_p < 1e-30:
            assert got[pos] < 1e-30
            continue
        check_logp(float(abs(np.log(got[pos]) - np.log(ref_p))), lgs[pos], None, pos)
    gm.close()
    om.close()


@pytest.mark.parametrize("name", sorted(DTS))
def test_synthetic_forward_at_4096(name):
    """dim 4096: qkv, W1/W3 and the lm_head take the GQ shape under the rmsnorm prologue, W2 (8192)
    the GQL shape; the device's synthetic fill equals the host quantizer over the same values."""
    dtype = DTS[name]
    for role in (L.ROLE_QKV, L.ROLE_GLU, L.ROLE_LOGITS, 5):  # 5: the qkv role writing an fp8 KV ring
        assert L.SHAPE_NAMES[L.gemv_shape(role, dtype, 4096)] == "GQ"
        assert L.SHAPE_NAMES[L.gemv_shape(role, dtype, 512)] == "Short"
    assert L.SHAPE_NAMES[L.gemv_shape(L.ROLE_RESID, dtype, 8192)] == "GQL"
    w = dict(dim=4096, hidden=8192, layers=1, heads=16, kv_heads=4, head_dim=128, vocab=1000, msl=256,
             theta=1e6, wdt=dtype, edt=dtype, cdt=dtype)
    c = bench.make_config(w)
    gm, om = Model(c), O.OracleModel(c)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
        gm.upload_synthetic(kind, layer, dt, seed, mean, std)
        rows, cols = bench.tensor_shape(c, kind)
        if dt == dtype:
            host = L.quantize_blocks(dt, O.synthetic(rows, cols, L.F32, seed, mean, std).reshape(rows, cols))
            om.set_tensor(kind, layer, L.F32, R.dequantize(dt, host))
        else:
            om.set_tensor(kind, layer, dt, O.synthetic(rows, cols, dt, seed, mean, std))
    st = InferenceState(c)
    for pos, tok in enumerate([1, 17, 999]):
        gm.forward(st, tok, pos)
        om.forward(tok, pos)
        ref = om.logits()
        assert np.abs(st.logits() - ref).max() <= north(ref), pos
    gm.close()
    om.close()


# ---- untouched formats --------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", ["tiny_mistral_q4_0", "tiny_mistral_q4_1", "tiny_mistral_mxfp4"])
def test_existing_formats_are_bit_identical_to_the_recorded_parent(fixture):
    """tests/golden/kq_unchanged.npz: 8 forward steps recorded from a build of the commit before the
    K-quants (tests/golden/make_kq_fixtures.py --unchanged)."""
    rec = np.load(fixture_path("kq_unchanged.npz"))[fixture]
    gm = Model.from_xalm(XalmFile(fixture_path(fixture + ".xalm")))
    st = InferenceState(gm.config)
    toks = [1] + [3 + (i * 37) % (gm.config.vocab_size - 3) for i in range(7)]
    for pos, tok in enumerate(toks):
        gm.forward(st, tok, pos)
        assert np.array_equal(st.logits().view(np.uint32), rec[pos].view(np.uint32)), (fixture, pos)
    gm.close()
