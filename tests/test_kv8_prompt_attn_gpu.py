"""The MFMA prompt attention over fp8 (e4m3) K/V: xh_op_prompt_attn8 and XH_OPT_PREFILL_ATTN_KV8.

Every finite e4m3 value is an f16 (tests/test_kv8_prompt_attn_cpu.py), so the attention over the
codes is by definition the fp16 prompt attention over their f16 image, and the fp8 kernels
(prefill_fa_kernel / prefill_fa2_kernel with KV = XH_F8_E4M3) are held to the fp16 kernels, which
tests/test_prompt_attn_gpu.py pins to a float64 reference, bit for bit: no tolerance.  Then one
case against the float64 reference itself under that file's bar, the rejections, and whole prompt
passes on fp8 contexts with the option on against tests/kv8_ref.py and against the option off."""
import ctypes
import functools

import numpy as np
import pytest

import bars
import bench
import kv8_ref as R
import prompt_attn_ref as PR
from conftest import fixture_path
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

F8 = L.F8_E4M3
E_INVALID = 1
TOKS = [1] + [3 + (i * 29) % 290 for i in range(47)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=8)
def rand_inputs(n_heads, n_kv, hd, n, pos0):
    """q ~ 0.5 N(0, 1) f32; K / V codes: the ring's rounding of N(0, 1)"""
    rng = np.random.default_rng([n_heads, n_kv, hd, n, pos0])
    q = (PR.Q_SCALE * rng.standard_normal((n, n_heads * hd))).astype(np.float32)
    k = L.f8_e4m3_from_f32(rng.standard_normal((pos0 + n, n_kv * hd)).astype(np.float32))
    v = L.f8_e4m3_from_f32(rng.standard_normal((pos0 + n, n_kv * hd)).astype(np.float32))
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


def both(q, k, v, pos0, hd, n_heads, n_kv, mode, nsplit):
    """(the fp8 kernel on the codes, the fp16 kernel on their image), same mode and splits"""
    got = L.op_prompt_attn8(q, k, v, pos0, hd, n_heads, n_kv, mode, nsplit)
    want = L.op_prompt_attn(q, R.image16(k), R.image16(v), pos0, hd, n_heads, n_kv, mode, nsplit)
    return got, want


def assert_bit_identical(got, want):
    assert np.all(np.isfinite(want))
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (bad.size, int(bad[0]), float(got.reshape(-1)[bad[0]]), float(want.reshape(-1)[bad[0]]))


# ---- 1. bit identity, op level --------------------------------------------------------------------
# mode 1 at head_dim 128 is the shared-tile kernel (one forced split: no merge); everything else the
# per-wave kernel, which takes no split count
def _ns(mode, hd):
    return 1 if mode == 1 and hd == 128 else 0


@pytest.mark.parametrize("pos0", [0, 1, 63, 64, 65, 300])
@pytest.mark.parametrize("n", [1, 31, 33, 70])
@pytest.mark.parametrize("mode", [1, 2])
def test_hd128_bit_identical_to_fp16_on_the_image(mode, n, pos0):
    """n: one row, a ragged workgroup tile (32 tokens at 4 q heads per KV head), one row into the
    second, and more than two; pos0: no history, stage edges (64 slots) and an odd stage count."""
    q, k, v = rand_inputs(8, 2, 128, n, pos0)
    assert_bit_identical(*both(q, k, v, pos0, 128, 8, 2, mode, _ns(mode, 128)))


@pytest.mark.parametrize("nsplit", [2, 4])
def test_forced_history_splits_bit_identical(nsplit):
    """the splits' partials and prefill_fa_merge_kernel behind the fp8 loader"""
    q, k, v = rand_inputs(8, 2, 128, 40, 1024)
    assert_bit_identical(*both(q, k, v, 1024, 128, 8, 2, 1, nsplit))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape", [(4, 4, 128), (8, 1, 128), (4, 4, 64), (4, 2, 64), (8, 1, 64), (4, 2, 16)], ids=str)
def test_head_shapes_bit_identical(shape, mode):
    """1 and 8 q heads per KV head at head_dim 128; the per-wave kernel's head_dim 64 and 16"""
    n_heads, n_kv, hd = shape
    q, k, v = rand_inputs(n_heads, n_kv, hd, 33, 65)
    assert_bit_identical(*both(q, k, v, 65, hd, n_heads, n_kv, mode, _ns(mode, hd)))


# ---- 2. every code at every position of a chunk ---------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_every_finite_code_in_every_lane_position(mode):
    """K and V rows cycle through the 254 finite codes (both zeros, the subnormals, +-448), the
    cycle shifted by one per row: over 256 rows every code stands at each of the 8 positions of a
    loader chunk.  q at 1/16 keeps the softmax from collapsing onto one key."""
    n, pos0, n_heads, n_kv, hd = 8, 248, 8, 2, 128
    rng = np.random.default_rng(254)
    q = (rng.standard_normal((n, n_heads * hd)) / 16).astype(np.float32)
    r, c = np.arange(pos0 + n)[:, None], np.arange(n_kv * hd)[None, :]
    k = R.FINITE[(c + r) % 254]
    v = R.FINITE[(c + r + 127) % 254]
    for a in (k, v):
        for e in range(8):
            assert set(np.unique(a[:, e::8])) == set(R.FINITE)
    got, want = both(q, k, v, pos0, hd, n_heads, n_kv, mode, _ns(mode, hd))
    assert_bit_identical(got, want)
    assert len(np.unique(bits(got))) > got.size // 2  # rows and heads differ: not one key's V row


# ---- 3. independent check -------------------------------------------------------------------------
def test_against_the_float64_reference_on_the_image():
    """the fp16 kernels' own bar (prompt_attn_ref.causal: DESIGN.md section 3), on the image"""
    n, pos0 = 33, 300
    q, k, v = rand_inputs(8, 2, 128, n, pos0)
    got = L.op_prompt_attn8(q, k, v, pos0, 128, 8, 2, 1, 1)
    ref, bar = PR.causal(q, R.image16(k), R.image16(v), pos0, 8, 2, 128)
    assert np.all(np.isfinite(got))
    r = float((np.abs(got.astype(np.float64) - ref) / bar).max())
    print(f"\nworst err / bar = {r:.4f}")
    assert r <= 1.0, r


# ---- 4. rejections --------------------------------------------------------------------------------
SENTINEL = 0x7FC0BEEF


def last_error():
    msg = L.lib().xh_last_error(None)
    return msg.decode() if msg else ""


def attn8_rc(k, v, n_heads, n_kv, hd, n, pos0, mode=1, nsplit=0):
    q = np.zeros((n, n_heads * hd), np.float32)
    out = np.full(q.shape, SENTINEL, np.uint32)
    rc = L.lib().xh_op_prompt_attn8(L.ptr(out), L.ptr(q), L.ptr(k), L.ptr(v), n, pos0, hd, n_heads, n_kv, mode, nsplit)
    return rc, out


@pytest.mark.parametrize("code", [0x7F, 0xFF])
@pytest.mark.parametrize("which", [0, 1])
def test_nan_code_is_rejected(code, which):
    kv = [np.zeros((12, 256), np.uint8), np.zeros((12, 256), np.uint8)]
    kv[which][11, 255] = code
    rc, out = attn8_rc(kv[0], kv[1], 8, 2, 128, 8, 4)
    assert rc == E_INVALID and "NaN" in last_error()
    assert np.all(out == SENTINEL)  # nothing ran


@pytest.mark.parametrize("args", [
    (6, 4, 128, 8, 0, 1, 0),      # 6 q heads over 4 KV heads
    (8, 2, 32, 8, 0, 1, 0),       # head_dim 32
    (16, 1, 128, 8, 0, 1, 0),     # 16 q heads per KV head
    (8, 2, 128, 8, 0, 0, 0),      # mode 0 is not this hook's
    (8, 2, 64, 8, 2400, 1, 2),    # splits under the per-wave kernel
], ids=str)
def test_prompt_attn8_rejects_what_prompt_attn_rejects(args):
    n_heads, n_kv, hd, n, pos0, mode, nsplit = args
    kv = np.zeros((pos0 + n, n_kv * hd), np.uint8)
    rc, out = attn8_rc(kv, kv, n_heads, n_kv, hd, n, pos0, mode, nsplit)
    assert rc == E_INVALID and last_error()
    assert np.all(out == SENTINEL)


def xalm(name):
    return XalmFile(fixture_path(name + ".xalm"))


@pytest.mark.parametrize("kv_dtype", [L.F16, F8])
def test_option_values(kv_dtype):
    gm = Model.from_xalm(xalm("tiny_mistral_f16"), kv_dtype=kv_dtype)
    assert L.OPT_PREFILL_ATTN_KV8 == 8 and gm.get_option(L.OPT_PREFILL_ATTN_KV8) == 0
    for bad in (2, -1):
        assert L.lib().xh_set_option(gm._ctx, L.OPT_PREFILL_ATTN_KV8, bad) == E_INVALID
        assert gm.get_option(L.OPT_PREFILL_ATTN_KV8) == 0
    gm.set_option(L.OPT_PREFILL_ATTN_KV8, 1)
    assert gm.get_option(L.OPT_PREFILL_ATTN_KV8) == 1
    assert gm.get_option(L.OPT_PREFILL_ATTN) == 1  # the other stored options are untouched
    gm.set_option(L.OPT_PREFILL_ATTN_KV8, 0)
    assert gm.get_option(L.OPT_PREFILL_ATTN_KV8) == 0
    gm.close()


# ---- 5. model level, the fixtures (head_dim 16 and 64: the per-wave kernel) -----------------------
def layer0_codes(gm, n):
    return gm.kv_read8(0, 0, 0, n).copy(), gm.kv_read8(0, 1, 0, n).copy()


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("name", ["tiny_mistral_f16", "small_llama_f16"])
def test_prefill_matches_reference(name, mode):
    xf = xalm(name)
    toks = TOKS[:40]
    g0 = Model.from_xalm(xf, context=256, kv_dtype=F8)
    g0.set_option(L.OPT_PREFILL, mode)
    route0 = g0.prefill_route(len(toks), 0)
    g0.prefill(toks, 0)
    codes0 = layer0_codes(g0, len(toks))
    g0.close()

    gm, ref = Model.from_xalm(xf, context=256, kv_dtype=F8), R.Kv8Ref(xf, context=256)
    gm.set_option(L.OPT_PREFILL, mode)
    gm.set_option(L.OPT_PREFILL_ATTN_KV8, 1)
    assert gm.prefill_route(len(toks), 0) == route0 and route0[0] == len(toks)  # the plan does not depend on it
    st = InferenceState(gm.config)
    gm.prefill(toks, 0, st)
    for pos, tok in enumerate(toks):
        want = ref.step(tok, pos, gm)  # verifies every layer's K/V codes, then adopts them
    err = float(np.abs(st.logits() - want).max())
    assert err <= bars.north(want), (name, mode, err, bars.north(want))
    assert ref.worst <= 1.0
    # layer 0's K/V are written before any attention: the option cannot move them
    codes1 = layer0_codes(gm, len(toks))
    assert np.array_equal(codes0[0], codes1[0]) and np.array_equal(codes0[1], codes1[1])


def logsoftmax(lg):
    lg = np.asarray(lg, np.float64)
    return lg - lg.max() - np.log(np.exp(lg - lg.max()).sum())


def test_score_matches_reference():
    xf = xalm("tiny_mistral_f16")
    gm, ref = Model.from_xalm(xf, context=256, kv_dtype=F8), R.Kv8Ref(xf, context=256)
    gm.set_option(L.OPT_PREFILL_ATTN_KV8, 1)
    toks = TOKS[:41]
    lp = gm.score(toks)["logprobs"]
    for pos, tok in enumerate(toks[:-1]):
        want = ref.step(tok, pos, gm)
        err = abs(float(lp[pos]) - float(logsoftmax(want)[toks[pos + 1]]))
        assert err <= 2 * bars.north(want) + 1e-5, (pos, err)  # the rule of bars.check_logp


# ---- 6. model level, head_dim 128 (the shared-tile kernel; no fixture has the shape) --------------
W128 = dict(dim=512, hidden=1024, layers=2, heads=4, kv_heads=1, head_dim=128, vocab=512, msl=512, theta=1e4,
            wdt=L.F16, edt=L.F16, cdt=L.F16)


def run128(option):
    gm = Model(bench.make_config(W128), 0, F8)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(W128):
        gm.upload_synthetic(kind, layer, dt, seed, mean, std)
    gm.set_option(L.OPT_PREFILL_ATTN_KV8, option)
    toks = bench.prompt_tokens(W128["vocab"], 240)
    st = InferenceState(gm.config)
    gm.prefill(toks[:200], 0)
    gm.prefill(toks[200:], 200, st)
    out = st.logits().copy(), layer0_codes(gm, 240), gm.prefill_route(40, 200)
    gm.close()
    return out


def test_head_dim_128_model_against_option_0():
    lg0, codes0, route0 = run128(0)
    lg1, codes1, route1 = run128(1)
    assert np.all(np.isfinite(lg0)) and np.all(np.isfinite(lg1)) and route0 == route1 == (40, route0[1])
    assert np.array_equal(codes0[0], codes1[0]) and np.array_equal(codes0[1], codes1[1])
    # both routes are held to north() of the same definition: their distance is at most twice it
    err = float(np.abs(lg1 - lg0).max())
    assert err <= 2 * bars.north(lg0), (err, bars.north(lg0))
    # the split merge is ordered: the route is deterministic
    assert np.array_equal(bits(run128(1)[0]), bits(lg1))
