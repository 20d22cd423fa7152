"""The fp8 (e4m3) KV ring on the device: the element's rounding against the host definition, the
attention over fp8 rings against the oracle on the codes' images, and whole forwards, prompt
passes, the ring wrap and the decode loops against tests/kv8_ref.py (verify, then adopt)."""
import ctypes

import numpy as np
import pytest

import bars
import kv8_ref as R
from conftest import fixture_path
from oracle import oracle as O
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

F8 = L.F8_E4M3
TOKS = [1] + [3 + (i * 29) % 290 for i in range(47)]


def xalm(name):
    return XalmFile(fixture_path(name + ".xalm"))


def logsoftmax(lg):
    lg = np.asarray(lg, np.float64)
    return lg - lg.max() - np.log(np.exp(lg - lg.max()).sum())


# ---- 2. the device quantizer is the host definition, bit for bit ---------------------------------
def test_kv_quantize_equals_host_definition():
    x = R.quantizer_inputs()
    got, want = L.op_kv_quantize(x), L.f8_e4m3_from_f32(x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(x[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    odd = x[:1001]  # an odd count: the last pair is half a pair
    assert np.array_equal(L.op_kv_quantize(odd), L.f8_e4m3_from_f32(odd))


# ---- 3. attention over fp8 rings ------------------------------------------------------------------
def mha8_case(rng, head_dim, n_heads, n_kv, kv_len, msl, kscale=1.0, qscale=0.5):
    kv_dim = n_kv * head_dim
    kb = L.f8_e4m3_from_f32((rng.standard_normal((msl, kv_dim)) * kscale).astype(np.float32))
    vb = L.f8_e4m3_from_f32(rng.standard_normal((msl, kv_dim)).astype(np.float32))
    q = (rng.standard_normal(n_heads * head_dim) * qscale).astype(np.float32)
    return kb, vb, q


def mha8_err(kb, vb, q, head_dim, n_heads, n_kv, kv_len, msl):
    got = L.op_mha8(kb, vb, q, head_dim, kv_len, msl, n_heads, n_kv)
    cpu = O.mha(R.image16(kb), R.image16(vb), q, head_dim, kv_len, msl, n_heads, n_kv)
    return float(np.abs(got - cpu).max())


@pytest.mark.parametrize("kv_len,msl", [(1, 64), (17, 64), (100, 128), (300, 4096), (4096, 4096)])
@pytest.mark.parametrize("head_dim,n_heads,n_kv", [(128, 32, 8), (128, 4, 1), (16, 4, 2), (64, 8, 8), (32, 8, 1),
                                                   (256, 16, 2)])
def test_mha8(head_dim, n_heads, n_kv, kv_len, msl):
    rng = np.random.default_rng(kv_len * 131 + head_dim + n_heads)
    err = mha8_err(*mha8_case(rng, head_dim, n_heads, n_kv, kv_len, msl), head_dim, n_heads, n_kv, kv_len, msl)
    assert err < 2e-5, err  # test_mha's bar: outputs are convex combinations of V rows


@pytest.mark.parametrize("n_heads,n_kv", [(32, 8), (8, 8), (16, 8)])
@pytest.mark.parametrize("kv_len", [257, 1000, 8191, 20001])
def test_mha8_long_splits(n_heads, n_kv, kv_len):
    rng = np.random.default_rng(kv_len + 7 * n_heads)
    err = mha8_err(*mha8_case(rng, 128, n_heads, n_kv, kv_len, 32768), 128, n_heads, n_kv, kv_len, 32768)
    assert err < 2e-5, err


def test_mha8_peaked_softmax_and_32k():
    rng = np.random.default_rng(5)
    head_dim, n_heads, n_kv, msl = 128, 32, 8, 32768
    kb, vb, q = mha8_case(rng, head_dim, n_heads, n_kv, msl, msl, kscale=0.3, qscale=1.0)
    kb[20000] = L.f8_e4m3_from_f32(np.tile(q[:head_dim] / np.linalg.norm(q[:head_dim]) * 8, n_kv).astype(np.float32))
    err = mha8_err(kb, vb, q, head_dim, n_heads, n_kv, msl, msl)
    assert err < 5e-5, err


# ---- 4. forward parity, verify-then-adopt ---------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_mistral_f16", "small_llama_f16", "tiny_mistral_f8_e4m3", "tiny_mistral_q4_0"])
def test_forward_matches_reference(name):
    xf = xalm(name)
    gm, ref = Model.from_xalm(xf, kv_dtype=F8), R.Kv8Ref(xf)
    assert gm.kv_dtype == F8
    st = InferenceState(gm.config)
    for pos, tok in enumerate(TOKS[:24]):
        gm.forward(st, tok, pos)
        want = ref.step(tok, pos, gm)
        err = float(np.abs(st.logits() - want).max())
        assert err <= bars.north(want), (name, pos, err, bars.north(want))
    assert ref.worst <= 1.0


# ---- 5. prompt passes -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("name", ["tiny_mistral_f16", "small_llama_f16"])
def test_prefill_matches_reference(name, mode):
    xf = xalm(name)
    gm, ref = Model.from_xalm(xf, context=256, kv_dtype=F8), R.Kv8Ref(xf, context=256)
    gm.set_option(L.OPT_PREFILL, mode)
    toks = TOKS[:40]
    # the plan is the attention-mode-0 plan of an fp16 context; the stored options read back as set
    g16 = Model.from_xalm(xf, context=256)
    g16.set_option(L.OPT_PREFILL, mode)
    g16.set_option(L.OPT_PREFILL_ATTN, 0)
    assert gm.prefill_route(len(toks), 0) == g16.prefill_route(len(toks), 0)
    assert gm.prefill_route(len(toks), 0)[0] == len(toks)
    assert gm.get_option(L.OPT_PREFILL_ATTN) == 1 and gm.get_option(L.OPT_PREFILL_RING) == 1
    g16.close()
    st = InferenceState(gm.config)
    gm.prefill(toks, 0, st)
    for pos, tok in enumerate(toks):
        want = ref.step(tok, pos, gm)
    err = float(np.abs(st.logits() - want).max())
    assert err <= bars.north(want), (name, mode, err, bars.north(want))


def test_score_matches_reference():
    xf = xalm("tiny_mistral_f16")
    gm, ref = Model.from_xalm(xf, context=256, kv_dtype=F8), R.Kv8Ref(xf, context=256)
    toks = TOKS[:41]
    lp = gm.score(toks)["logprobs"]
    for pos, tok in enumerate(toks[:-1]):
        want = ref.step(tok, pos, gm)
        err = abs(float(lp[pos]) - float(logsoftmax(want)[toks[pos + 1]]))
        assert err <= 2 * bars.north(want) + 1e-5, (pos, err)  # the rule of bars.check_logp


# ---- 6. ring wrap ---------------------------------------------------------------------------------
def test_ring_wrap_sinks_through_the_master():
    xf = xalm("tiny_mistral_f16")
    gm, ref = Model.from_xalm(xf, context=16, kv_dtype=F8), R.Kv8Ref(xf, context=16)
    st = InferenceState(gm.config)
    for pos, tok in enumerate(TOKS[:41]):
        gm.forward(st, tok, pos)
        want = ref.step(tok, pos, gm)  # past 16: master rows, ring slots 0 / 1 == f8(master), the new rows
        err = float(np.abs(st.logits() - want).max())
        assert err <= bars.north(want), (pos, err, bars.north(want))
    assert ref.worst <= 1.0
    # a prompt that crosses the ring's end batches only the part below it
    assert gm.prefill_route(20, 4)[0] == 12
    assert gm.prefill_route(8, 16) == (0, 0)


# ---- 7. loops -------------------------------------------------------------------------------------
def prompt_ctx(xf, graphs, n_prompt=6):
    gm = Model.from_xalm(xf, kv_dtype=F8)
    gm.set_graphs(graphs)
    st = InferenceState(gm.config)
    for pos, tok in enumerate(TOKS[:n_prompt]):
        gm.forward(st, tok, pos)
    return gm, st


@pytest.mark.parametrize("graphs", [True, False])
def test_decode_greedy_equals_forward_argmax(graphs):
    xf, n0 = xalm("tiny_mistral_f16"), 6
    gm, st = prompt_ctx(xf, graphs)
    want = []
    for i in range(24):
        want.append(O.sample_argmax(st.logits()))
        gm.forward(st, want[-1], n0 + i)
    gm.close()
    gm, _ = prompt_ctx(xf, graphs)
    assert gm.decode_greedy(n0, 24) == want
    gm.close()
    gm, _ = prompt_ctx(xf, graphs)
    assert gm.decode_greedy(n0, 12) + gm.decode_greedy(n0 + 12, 12) == want


def test_decode_sample_graphs_on_off():
    xf, out = xalm("tiny_mistral_f16"), []
    for graphs in (True, False):
        gm, _ = prompt_ctx(xf, graphs)
        out.append(gm.decode_sample(6, 24, 0.8, top_k=20, top_p=0.9, seed=7))
        gm.close()
    assert len(out[0]) == 24 and out[0] == out[1]


# ---- 8. the fp16 path is untouched ----------------------------------------------------------------
class ModelPlainCreate(Model):
    def __init__(self, config, device=0, kv_dtype=L.F16):
        self.config = config
        self._ctx = ctypes.c_void_p()
        L.check(L.lib().xh_create(ctypes.byref(config), device, ctypes.byref(self._ctx)))


def test_create_kv_f16_is_create():
    xf = xalm("tiny_mistral_f16")
    a, b = ModelPlainCreate.from_xalm(xf), Model.from_xalm(xf, kv_dtype=L.F16)
    assert a.kv_dtype == L.F16 and b.kv_dtype == L.F16
    sa, sb = InferenceState(a.config), InferenceState(b.config)
    for pos, tok in enumerate(TOKS[:8]):
        a.forward(sa, tok, pos)
        b.forward(sb, tok, pos)
        assert np.array_equal(sa.logits().view(np.uint32), sb.logits().view(np.uint32)), pos
    for l in range(a.config.n_layers):
        for which in (0, 1):
            assert np.array_equal(a.kv_read(l, which, 0, 8), b.kv_read(l, which, 0, 8))


# ---- 9. rejections and the IO ---------------------------------------------------------------------
def test_rejections_and_io():
    xf = xalm("tiny_mistral_f16")
    cfg = xf.config()
    inv = 1  # XH_E_INVALID
    ctx = ctypes.c_void_p()
    for bad in (L.BF16, L.F8_E5M2, 0, 99):
        assert L.lib().xh_create_kv(ctypes.byref(cfg), 0, bad, ctypes.byref(ctx)) == inv and not ctx
    c8 = xf.config()
    c8.head_dim = 8
    assert L.lib().xh_create_kv(ctypes.byref(c8), 0, F8, ctypes.byref(ctx)) == inv and not ctx

    g8, g16 = Model.from_xalm(xf, kv_dtype=F8), Model.from_xalm(xf)
    kv_dim, msl = cfg.n_kv_heads * cfg.head_dim, cfg.max_seq_len
    lib = L.lib()
    rng = np.random.default_rng(3)
    rows = R.FINITE[rng.integers(0, 254, (4, kv_dim))]
    g8.kv_write8(0, 0, 0, rows)
    g8.kv_write8(0, 1, 5, rows)
    before = (g8.kv_read8(0, 0, 0, msl).copy(), g8.kv_read8(0, 1, 0, msl).copy(), g8.kv_sink_read(0).copy())
    assert np.array_equal(before[0][:4], rows) and np.array_equal(before[1][5:9], rows)  # round trip
    assert np.array_equal(before[2], R.image16(rows[:2]))  # K slots 0..1 are visible as the exact image
    assert not g8.kv_read8(0, 1, 0, 2).any() and not g8.kv_sink_read(1).any()  # V rows and other layers: no master

    buf16, buf8 = np.zeros((2, kv_dim), np.uint16), np.zeros((2, kv_dim), np.uint8)
    assert lib.xh_kv_write(g8._ctx, 0, 0, 0, 2, L.ptr(buf16)) == inv
    assert lib.xh_kv_read(g8._ctx, 0, 0, 0, 2, L.ptr(buf16)) == inv
    nan = rows[:2].copy()
    nan[1, 7] = 0xFF
    assert lib.xh_kv_write8(g8._ctx, 0, 0, 0, 2, L.ptr(nan)) == inv
    nan[1, 7] = 0x7F
    assert lib.xh_kv_write8(g8._ctx, 0, 0, 0, 2, L.ptr(nan)) == inv
    assert lib.xh_kv_write8(g8._ctx, 0, 0, msl - 1, 2, L.ptr(buf8)) == inv  # out-of-range slots
    assert lib.xh_kv_read8(g8._ctx, 0, 0, msl - 1, 2, L.ptr(buf8)) == inv
    assert lib.xh_kv_write8(g8._ctx, cfg.n_layers, 0, 0, 2, L.ptr(buf8)) == inv
    assert lib.xh_kv_sink_read(g8._ctx, cfg.n_layers, L.ptr(buf16)) == inv
    after = (g8.kv_read8(0, 0, 0, msl), g8.kv_read8(0, 1, 0, msl), g8.kv_sink_read(0))
    assert all(np.array_equal(x, y) for x, y in zip(before, after))  # nothing was touched

    k16 = g16.kv_read(0, 0, 0, 4).copy()
    assert lib.xh_kv_write8(g16._ctx, 0, 0, 0, 2, L.ptr(buf8)) == inv
    assert lib.xh_kv_read8(g16._ctx, 0, 0, 0, 2, L.ptr(buf8)) == inv
    assert lib.xh_kv_sink_read(g16._ctx, 0, L.ptr(buf16)) == inv
    assert np.array_equal(g16.kv_read(0, 0, 0, 4), k16)

    # the synthetic fill stores the e4m3 rounding of the fp16 fill's value, the master likewise
    g8.kv_fill_synthetic(1, 0, 0, 6, 900, 1.0)
    g16.kv_fill_synthetic(1, 0, 0, 6, 900, 1.0)
    want = L.f8_e4m3_from_f32(g16.kv_read(1, 0, 0, 6).view(np.float16).astype(np.float32))
    assert np.array_equal(g8.kv_read8(1, 0, 0, 6), want)
    assert np.array_equal(g8.kv_sink_read(1), R.image16(want[:2]))

    g8.reset()
    assert not g8.kv_read8(0, 0, 0, msl).any() and not g8.kv_read8(1, 0, 0, msl).any()
    assert not g8.kv_sink_read(0).any() and not g8.kv_sink_read(1).any()

    for pos in (0, 7, msl + 5):
        kv_len = min(pos + 1, msl)
        assert g16.active_bytes(pos) - g8.active_bytes(pos) == cfg.n_layers * 2 * kv_len * kv_dim
    assert g8.kernel_bytes(5, 100) == g16.kernel_bytes(5, 100) - 2 * 100 * kv_dim
