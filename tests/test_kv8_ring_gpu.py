"""Ring passes on the fp8 (e4m3) KV ring: xh_op_prompt_attn_ring8 and XH_OPT_PREFILL_RING_KV8.

Op level.  Every finite e4m3 value is an f16 (tests/test_kv8_prompt_attn_cpu.py), so the ring pass
over codes is by definition the fp16 ring pass over their f16 image, and the fp8 forms
(prefill_fa2_ring_kernel with KV = XH_F8_E4M3, prefill_fa_merge_kernel<true, XH_F8_E4M3>, the fp8
commit) are held to the fp16 kernels, which tests/test_prompt_attn_gpu.py pins to a float64
reference, bit for bit: no tolerance.  Then one case against the float64 reference itself under
that file's bar, and the rejections.

Model level.  The definition is the token loop on an fp8 context (rotate_sinks<THREADS, true>,
EPI_QKV8): context A (XH_OPT_PREFILL_ATTN_KV8 1, XH_OPT_PREFILL_RING_KV8 1) against context B (the
same with XH_OPT_PREFILL_RING_KV8 0, the loop past max_seq_len) on the same weights and ring.  Both
routes are held to bars.north() of one definition, so their logits differ by at most twice it; the
sink masters are one function iterated on the same bits and agree bit for bit.
"""
import functools

import numpy as np
import pytest

import bars
import bench
import kv8_ref as R
import prompt_attn_ref as PR
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model

pytestmark = pytest.mark.gpu

F8 = L.F8_E4M3
E_INVALID = 1
SENTINEL = 0x7FC0BEEF


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def codes_of(rng, shape):
    """the ring's rounding of N(0, 1)"""
    x = rng.standard_normal(int(np.prod(shape))).astype(np.float32)
    return L.f8_e4m3_from_f32(x).reshape(shape)


@functools.lru_cache(maxsize=8)
def rand_inputs(n_heads, n_kv, Lr, p0, m):
    """q ~ 0.5 N(0, 1) f32; the five code buffers: the ring's rounding of N(0, 1)"""
    rng = np.random.default_rng([n_heads, n_kv, Lr, p0, m])
    kv = n_kv * 128
    q = (PR.Q_SCALE * rng.standard_normal((m, n_heads * 128))).astype(np.float32)
    out = [q] + [codes_of(rng, s) for s in ((Lr, kv), (Lr, kv), (m, kv), (m, kv), (m, 2, kv))]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def assert_bit_identical(got, want):
    assert np.all(np.isfinite(want))
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (bad.size, int(bad[0]), float(got.reshape(-1)[bad[0]]), float(want.reshape(-1)[bad[0]]))


def both(inp, p0, n_heads, n_kv, nsplit):
    """The fp8 hook on the codes against the fp16 hook on their image, same splits: `out` by f32 bits,
    the returned rings as codes against the fp16 hook's returned rings; every ring row the pass does
    not map to (V rows 0 and 1 among them) unchanged.  Returns the fp8 hook's out."""
    q, kr, vr, ks, vs, sv = inp
    got, k2, v2 = L.op_prompt_attn_ring8(q, kr, vr, ks, vs, sv, p0, n_heads, n_kv, nsplit)
    want, wk, wv = L.op_prompt_attn_ring(q, R.image16(kr), R.image16(vr), R.image16(ks), R.image16(vs), R.image16(sv),
                                         p0, n_heads, n_kv, nsplit)
    assert_bit_identical(got, want)
    assert k2.dtype == np.uint8 and v2.dtype == np.uint8
    assert np.array_equal(R.image16(k2), wk) and np.array_equal(R.image16(v2), wv)
    m, Lr = ks.shape[0], kr.shape[0]
    mapped = PR.ring_slots(p0, Lr, m)
    rest = np.setdiff1d(np.arange(2, Lr), mapped)
    assert rest.size == Lr - 2 - m
    assert np.array_equal(k2[rest], kr[rest]) and np.array_equal(v2[rest], vr[rest])
    assert np.array_equal(v2[:2], vr[:2])
    assert np.array_equal(k2[mapped], ks) and np.array_equal(v2[mapped], vs) and np.array_equal(k2[:2], sv[m - 1])
    return got


# ---- 1. bit identity, op level --------------------------------------------------------------------
@pytest.mark.parametrize("p0", [160, 2 * 160 - 12])
@pytest.mark.parametrize("m", [3, 33, 158])
def test_bit_identical_to_fp16_on_the_image(m, p0):
    """L = 160 (W = 158, no multiple of a tile), 8 q heads over 2 KV heads.  m: the minimum, one row
    into a second wave tile, the full-length pass whose last row sees no history; p0: hoff 0, and a
    pass that writes across the physical wrap from slot L - 1 to slot 2."""
    both(rand_inputs(8, 2, 160, p0, m), p0, 8, 2, 1)


@pytest.mark.parametrize("nsplit", [2, 4])
def test_forced_splits_bit_identical(nsplit):
    """L = 1026 (W = 1024: up to 4 splits): the split partials and the merge with the sinks behind the
    fp8 loader, splits invisible to some rows included"""
    p0 = 2 * 1026 - 12
    both(rand_inputs(8, 2, 1026, p0, 40), p0, 8, 2, nsplit)


@pytest.mark.parametrize("shape", [(4, 4), (8, 1)], ids=str)
def test_head_shapes_bit_identical(shape):
    """1 and 8 q heads per KV head"""
    p0 = 2 * 160 - 12
    both(rand_inputs(*shape, 160, p0, 33), p0, *shape, 1)


# ---- 2. every code at every position of a chunk ---------------------------------------------------
def test_every_finite_code_in_every_lane_position():
    """Ring rows, staging rows and sink versions cycle through the 254 finite codes (both zeros, the
    subnormals, +-448), the cycle shifted by one per row: over the 256 history rows, and over the 8
    staging rows of 256 columns, every code stands at each of the 8 positions of a loader chunk.  q at
    1/16 keeps the softmax from collapsing onto one key."""
    Lr, m, n_heads, n_kv = 258, 8, 8, 2
    p0 = 2 * Lr - 12
    kv = n_kv * 128
    rng = np.random.default_rng(254)
    q = (rng.standard_normal((m, n_heads * 128)) / 16).astype(np.float32)
    r, c = np.arange(Lr)[:, None], np.arange(kv)[None, :]
    kr, vr = R.FINITE[(c + r) % 254], R.FINITE[(c + r + 127) % 254]
    t = np.arange(m)[:, None]
    ks, vs = R.FINITE[(c + t + 31) % 254], R.FINITE[(c + t + 158) % 254]
    sv = R.FINITE[(np.arange(kv)[None, None, :] + 2 * np.arange(m)[:, None, None] + np.arange(2)[None, :, None] + 60) % 254]
    for a in (kr[2:], vr[2:], ks, vs, sv.reshape(2 * m, kv)):
        for e in range(8):
            assert set(np.unique(a[:, e::8])) == set(R.FINITE)
    got = both((q, kr, vr, ks, vs, sv), p0, n_heads, n_kv, 1)
    assert len(np.unique(bits(got))) > got.size // 2  # rows and heads differ: not one key's V row


# ---- 3. independent check -------------------------------------------------------------------------
def test_against_the_float64_reference_on_the_image():
    """the fp16 ring kernel's own bar (prompt_attn_ref.ring: DESIGN.md section 3), on the image; the wrap
    inside the pass; the rings against the reference's exact moves"""
    p0, m = 2 * 160 - 12, 33
    q, kr, vr, ks, vs, sv = rand_inputs(8, 2, 160, p0, m)
    got, k2, v2 = L.op_prompt_attn_ring8(q, kr, vr, ks, vs, sv, p0, 8, 2, 1)
    ref, bar = PR.ring(q, R.image16(kr), R.image16(vr), R.image16(ks), R.image16(vs), R.image16(sv), p0, 8, 2)
    assert np.all(np.isfinite(got))
    r = float((np.abs(got.astype(np.float64) - ref) / bar).max())
    print(f"\nworst err / bar = {r:.4f}")
    assert r <= 1.0, r
    want_k, want_v = PR.ring_after_commit(kr, vr, ks, vs, sv, p0)
    assert np.array_equal(k2, want_k) and np.array_equal(v2, want_v)


# ---- 4. rejections --------------------------------------------------------------------------------
def last_error():
    msg = L.lib().xh_last_error(None)
    return msg.decode() if msg else ""


def ring8_rc(bufs, m, p0, Lr, n_heads=8, n_kv=2, nsplit=1):
    kr, vr, ks, vs, sv = bufs
    q = np.zeros((max(m, 1), n_heads * 128), np.float32)
    out = np.full(q.shape, SENTINEL, np.uint32)
    rc = L.lib().xh_op_prompt_attn_ring8(L.ptr(out), L.ptr(kr), L.ptr(vr), L.ptr(q), L.ptr(ks), L.ptr(vs), L.ptr(sv), m, p0,
                                         Lr, n_heads, n_kv, nsplit)
    return rc, out


def zero_bufs(Lr, m, kv=256, fill=0x38):
    return [np.full((Lr, kv), fill, np.uint8), np.full((Lr, kv), fill, np.uint8), np.zeros((m, kv), np.uint8),
            np.zeros((m, kv), np.uint8), np.zeros((m, 2, kv), np.uint8)]


@pytest.mark.parametrize("code", [0x7F, 0xFF])
@pytest.mark.parametrize("which", range(5), ids=["k_ring", "v_ring", "ks", "vs", "sink_ver"])
def test_nan_code_is_rejected(which, code):
    bufs = zero_bufs(66, 8)
    bufs[which].reshape(-1)[-1] = code
    before = [b.copy() for b in bufs]
    rc, out = ring8_rc(bufs, 8, 66, 66)
    assert rc == E_INVALID and "NaN" in last_error()
    assert np.all(out == SENTINEL)  # nothing ran
    assert all(np.array_equal(a, b) for a, b in zip(bufs, before))


@pytest.mark.parametrize("L_,p0,m,heads,nsplit", [
    (66, 66, 2, (8, 2), 1),      # m < 3
    (66, 66, 65, (8, 2), 1),     # m = W + 1
    (66, 65, 8, (8, 2), 1),      # p0 < L
    (3, 66, 3, (8, 2), 1),       # W < 2
    (66, 66, 8, (6, 4), 1),
    (66, 66, 8, (8, 2), 2),      # W / 64 / 4 = 0: one split
    (2306, 3306, 8, (8, 2), 10),
], ids=str)
def test_rejects_what_the_fp16_hook_rejects(L_, p0, m, heads, nsplit):
    n_heads, n_kv = heads
    bufs = zero_bufs(max(L_, 1), max(m, 1), n_kv * 128)
    rc, out = ring8_rc(bufs, m, p0, L_, n_heads, n_kv, nsplit)
    assert rc == E_INVALID and last_error()
    assert np.all(out == SENTINEL) and np.all(bufs[0] == 0x38) and np.all(bufs[1] == 0x38)


# ---- 5. model level (head_dim 128: no fixture has the shape) ---------------------------------------
W128 = dict(dim=512, hidden=1024, layers=2, heads=4, kv_heads=1, head_dim=128, vocab=512, theta=1e4,
            wdt=L.F16, edt=L.F16, cdt=L.F16)
KV_DIM = 128
FILL_SEED = 4100


def make(msl, ring_kv8, kv_dtype=F8, attn_kv8=1):
    w = dict(W128, msl=msl)
    gm = Model(bench.make_config(w), 0, kv_dtype)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
        gm.upload_synthetic(kind, layer, dt, seed, mean, std)
    gm.set_option(L.OPT_PREFILL_ATTN_KV8, attn_kv8)
    gm.set_option(L.OPT_PREFILL_RING_KV8, ring_kv8)
    return gm


def fill(gm, msl):
    for layer in range(W128["layers"]):
        for which in (0, 1):
            gm.kv_fill_synthetic(layer, which, 0, msl, FILL_SEED + 2 * layer + which, 1.0)


def ring_codes(gm, msl):
    """[layer][which] -> codes [msl][kv_dim]"""
    return [[gm.kv_read8(layer, which, 0, msl).copy() for which in (0, 1)] for layer in range(W128["layers"])]


def masters(gm):
    return [gm.kv_sink_read(layer).copy() for layer in range(W128["layers"])]


def f8_of_master(master):
    return L.f8_e4m3_from_f32(np.ascontiguousarray(master).view(np.float16).astype(np.float32).reshape(-1)).reshape(master.shape)


def within_twice_north(a, b, what=""):
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    err = float(np.abs(a - b).max())
    print(f"\n{what}: |A - B| = {err:.3e}, 2 north(B) = {2 * bars.north(b):.3e}")
    assert err <= 2 * bars.north(b), (what, err, 2 * bars.north(b))


ROUTE_ARGS = [((400, 0), (400, 3)), ((163, 0), (163, 2)), ((162, 0), (160, 1)), ((3, 200), (3, 1)), ((2, 200), (0, 0))]


def test_route_and_option_values():
    msl = 160
    a, b, h = make(msl, 1), make(msl, 0), make(msl, 0, L.F16, 0)
    assert L.OPT_PREFILL_RING_KV8 == 9 and b.get_option(L.OPT_PREFILL_RING_KV8) == 0
    assert a.get_option(L.OPT_PREFILL_RING_KV8) == 1
    # A plans as an fp16 context of the same configuration plans
    for args, want in ROUTE_ARGS:
        assert a.prefill_route(*args) == want == h.prefill_route(*args), args
    # B as ever: batched below L, the loop from the cut
    assert b.prefill_route(400, 0) == (160, 1) and b.prefill_route(8, 160) == (0, 0)
    # the option needs the fp8 MFMA attention and the ring passes' own option
    for opt in (L.OPT_PREFILL_ATTN_KV8, L.OPT_PREFILL_RING):
        a.set_option(opt, 0)
        assert a.prefill_route(400, 0) == (160, 1) and a.prefill_route(8, 160) == (0, 0), opt
        assert a.get_option(L.OPT_PREFILL_RING_KV8) == 1  # stored, ignored
        a.set_option(opt, 1)
    a.set_option(L.OPT_PREFILL_ATTN, 2)  # ring passes need the shared-tile attention
    assert a.prefill_route(400, 0) == (160, 1)
    a.set_option(L.OPT_PREFILL_ATTN, 1)
    assert a.prefill_route(400, 0) == (400, 3)
    for bad in (2, -1):
        assert L.lib().xh_set_option(a._ctx, L.OPT_PREFILL_RING_KV8, bad) == E_INVALID
        assert a.get_option(L.OPT_PREFILL_RING_KV8) == 1
        assert L.lib().xh_set_option(b._ctx, L.OPT_PREFILL_RING_KV8, bad) == E_INVALID
        assert b.get_option(L.OPT_PREFILL_RING_KV8) == 0
    # an fp16 context stores the value, reads it back and routes as before
    before = [h.prefill_route(*args) for args, _ in ROUTE_ARGS]
    h.set_option(L.OPT_PREFILL_RING_KV8, 1)
    assert h.get_option(L.OPT_PREFILL_RING_KV8) == 1
    assert [h.prefill_route(*args) for args, _ in ROUTE_ARGS] == before
    for gm in (a, b, h):
        gm.close()


@functools.lru_cache(maxsize=1)
def crossing():
    """msl 160, one prefill of 400 tokens at pos 0 with logits, on A and B (and on A2, a second A, for
    the teacher-forced steps); before it a run cut at 160 for the sink rows at position 159."""
    msl, n = 160, 400
    toks = bench.prompt_tokens(W128["vocab"], n)
    out = {"toks": toks, "msl": msl}
    for name, ring_kv8 in (("A", 1), ("B", 0), ("A2", 1)):
        gm = make(msl, ring_kv8)
        st = InferenceState(gm.config)
        gm.prefill(toks[:msl], 0)
        at159 = masters(gm)
        gm.reset()
        assert gm.prefill_route(n, 0) == ((400, 3) if ring_kv8 else (160, 1))
        gm.prefill(toks, 0, st)
        out[name] = dict(gm=gm, st=st, logits=st.logits().copy(), codes=ring_codes(gm, msl), masters=masters(gm),
                         at159=at159)
    return out


def test_crossing_prompt():
    x = crossing()
    a, b = x["A"], x["B"]
    for layer in range(W128["layers"]):
        # the same function iterated 240 times on the same bits, where the sink rows agreed at the cut
        # (layer 0's are written before any attention: always)
        same_start = np.array_equal(a["at159"][layer], b["at159"][layer])
        assert same_start or layer > 0
        if same_start:
            assert np.array_equal(a["masters"][layer], b["masters"][layer]), layer
        assert not np.array_equal(a["masters"][layer], a["at159"][layer])
        # ring K slot r == f8(master[r]) on both routes
        for side in (a, b):
            assert np.array_equal(side["codes"][layer][0][:2], f8_of_master(side["masters"][layer])), layer
    # layer 0's K/V are written before any attention
    for which in (0, 1):
        assert np.array_equal(a["codes"][0][which], b["codes"][0][which]), which
    within_twice_north(a["logits"], b["logits"], "crossing")


def test_decode_continues():
    """6 device greedy steps on A after the crossing prompt; the same tokens teacher-forced through A2's
    and B's forward agree step by step, and A's last logits agree with B's"""
    x = crossing()
    a, a2, b = x["A"], x["A2"], x["B"]
    nxt = a["gm"].decode_greedy(400, 6)
    assert len(nxt) == 6
    for i, t in enumerate(nxt):
        a2["gm"].forward(a2["st"], t, 400 + i)
        b["gm"].forward(b["st"], t, 400 + i)
        within_twice_north(a2["st"].logits(), b["st"].logits(), f"step {i}")
    a["gm"].get_logits(a["st"])
    within_twice_north(a["st"].logits(), b["st"].logits(), "after the device loop")


@pytest.mark.parametrize("n", [3, 4, 35])
def test_pass_lengths_from_one_filled_ring(n):
    """The final sink version of a pass of t + 1 tokens is the version token t of a longer pass scores
    against: the three lengths pin the intermediate versions to the token loop's."""
    msl, p0 = 160, 1000
    toks = bench.prompt_tokens(W128["vocab"], n)
    got = {}
    for name, ring_kv8 in (("A", 1), ("B", 0)):
        gm = make(msl, ring_kv8)
        fill(gm, msl)
        start = masters(gm)
        assert gm.prefill_route(n, p0) == ((n, 1) if ring_kv8 else (0, 0))
        gm.prefill(toks, p0)
        got[name] = (masters(gm), ring_codes(gm, msl))
        assert not np.array_equal(got[name][0][0], start[0])
        gm.close()
    (ma, ca), (mb, cb) = got["A"], got["B"]
    assert np.array_equal(ma[0], mb[0])
    assert np.array_equal(ca[0][0][:2], cb[0][0][:2]) and np.array_equal(ca[0][0][:2], f8_of_master(ma[0]))


def test_long_history_with_splits():
    """msl 4096, the ring full, 64 tokens at pos0 5000: the window walk in splits"""
    msl, p0, n = 4096, 5000, 64
    toks = bench.prompt_tokens(W128["vocab"], n)
    s0 = 2 + (p0 - 2) % (msl - 2)
    assert s0 + n <= msl
    res = {}
    for name, ring_kv8 in (("A", 1), ("B", 0), ("A again", 1)):
        gm = make(msl, ring_kv8)
        fill(gm, msl)
        filled = ring_codes(gm, msl)
        assert gm.prefill_route(n, p0) == ((n, 1) if ring_kv8 else (0, 0))
        st = InferenceState(gm.config)
        gm.prefill(toks, p0, st)
        res[name] = (st.logits().copy(), ring_codes(gm, msl))
        for layer in range(W128["layers"]):
            for which in (0, 1):
                lo = 2 if which == 0 else 0  # V's sink rows are never written
                now = res[name][1][layer][which]
                assert np.array_equal(now[lo:s0], filled[layer][which][lo:s0]), (name, layer, which)
                assert np.array_equal(now[s0 + n:], filled[layer][which][s0 + n:]), (name, layer, which)
        gm.close()
    within_twice_north(res["A"][0], res["B"][0], "long history")
    for which in (0, 1):
        assert np.array_equal(res["A"][1][0][which][s0:s0 + n], res["B"][1][0][which][s0:s0 + n]), which
    assert np.array_equal(bits(res["A again"][0]), bits(res["A"][0]))  # the merge is ordered


def test_token_probs_and_score_across_the_wrap():
    msl, n = 160, 200
    toks = bench.prompt_tokens(W128["vocab"], n)
    a, b = make(msl, 1), make(msl, 0)
    sb = b.score(toks, echo_logits=True)
    b.reset()
    pb = b.token_probs(toks)
    sa = a.score(toks)
    a.reset()
    pa = a.token_probs(toks)
    skipped = 0
    for pos in range(n - 1):
        lg = sb["logits"][pos]
        if pb[pos] < 1e-30:
            assert pa[pos] < 1e-30, (pos, pa[pos], pb[pos])
            skipped += 1
            continue
        assert pa[pos] > 0, (pos, pa[pos], pb[pos])
        bars.check_logp(float(abs(np.log(pa[pos]) - np.log(pb[pos]))), lg, None, ("token_probs", pos))
        bars.check_logp(float(abs(float(sa["logprobs"][pos]) - float(sb["logprobs"][pos]))), lg, None, ("score", pos))
    assert skipped <= (n - 1) // 4, skipped
    a.close()
    b.close()
