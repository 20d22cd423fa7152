"""Batched prompt passes across the KV ring wrap (XH_OPT_PREFILL_RING, prefill_fa2_ring_kernel).

From position L = max_seq_len on the reference keeps two sink slots, writes token p to slot
2 + (p - 2) % (L - 2), re-rotates the sink K rows by rope(pos = 1) before every step's attention
and attends over all L slots (src/infer.cpp:608-613, :416-431).  xh_prefill / xh_perplexity cut a
prompt at L and run the part from there on as ring passes.  The reference of every comparison is
the oracle's token loop on the same weights and ring contents.  Bars: logits 1e-3 max(1, max|ref|),
K/V rows 2e-3 max(1, max|ref|), log-probabilities tests/bars.py::check_logp.
"""
import numpy as np
import pytest

from bars import check_logp
from conftest import fixture_path
from oracle import oracle as O
from test_regimes_gpu import bar, build_pair, check_teacher_forced, f16, make_cfg
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu


def base_cfg(msl, heads=8, kv_heads=2):
    return make_cfg(256, 512, 2, heads, kv_heads, 128, 512, msl)


def tokens(n, mul=37):
    return [1] + [3 + (i * mul) % 500 for i in range(n - 1)]


def fill(gm, om, c, n_slots, seed0):
    """Synthetic K/V in slots [0, n_slots) of every layer, the same on both sides (om may be None)."""
    kv_dim = c.n_kv_heads * c.head_dim
    for layer in range(c.n_layers):
        for which in (0, 1):
            seed = seed0 + 2 * layer + which
            gm.kv_fill_synthetic(layer, which, 0, n_slots, seed, 1.0)
            if om is not None:
                om.set_kv(layer, which, 0, O.synthetic(n_slots, kv_dim, L.F16, seed, 0.0, 1.0))


def oracle_loop(om, toks, pos0):
    for i, t in enumerate(toks):
        om.forward(t, pos0 + i, L.OUTPUT_LOGITS if i == len(toks) - 1 else L.HYDRATE_KV_CACHE)
    return om.logits().copy()


def check_rows(gm, om, c, slots, what=""):
    """Ring rows `slots` (a list of (slot0, n)) of K and V in every layer against the oracle's."""
    for layer in range(c.n_layers):
        for which in (0, 1):
            for s0, n in slots:
                a = f16(gm.kv_read(layer, which, s0, n))
                b = f16(om.kv(layer, which)[s0:s0 + n])
                err = float(np.abs(a - b).max())
                assert err <= 2e-3 * max(1.0, float(np.abs(b).max())), (what, layer, which, s0, err)


def check_logits(got, ref, what=""):
    err = float(np.abs(got - ref).max())
    assert err <= bar(ref), (what, err, bar(ref))


def kv_pos(pos, msl):
    return 2 + (pos - 2) % (msl - 2)


# 1 ------------------------------------------------------------------------------------------
def test_route():
    """The cutting rule, as the launcher itself evaluates it (xh_prefill_route): a prompt is cut
    at L; below it the passes of old, from it on ring passes of at most L - 2 tokens; one or two
    tokens there, alone or left over by the ring passes, take the token loop (two decode steps
    measured faster than a pass of two); XH_OPT_PREFILL_RING 0 sends any prompt that reaches past L
    to the loop as a whole."""
    msl = 160
    c = base_cfg(msl)
    gm, om = build_pair(c, L.F16)
    om.close()
    assert L.OPT_PREFILL_RING == 7 and gm.get_option(L.OPT_PREFILL_RING) == 1
    assert gm.prefill_route(400, 0) == (400, 3)        # 160 in one pass | 158 + 82
    assert gm.prefill_route(100, 0) == (100, 1)        # inside the ring: as ever
    assert gm.prefill_route(160, 0) == (160, 1)
    assert gm.prefill_route(1, 0) == (0, 0)            # the one-token rule
    assert gm.prefill_route(161, 0) == (160, 1)        # one token past L: the loop
    assert gm.prefill_route(162, 0) == (160, 1)        # two tokens past L: the loop
    assert gm.prefill_route(163, 0) == (163, 2)
    assert gm.prefill_route(160 + 159, 0) == (318, 2)  # 158, then one left over: the loop
    assert gm.prefill_route(160 + 160, 0) == (318, 2)  # ... two left over
    assert gm.prefill_route(160 + 161, 0) == (321, 3)
    assert gm.prefill_route(4, 159) == (3, 1)          # one token below L (the loop), three from L on
    assert gm.prefill_route(1, 200) == (0, 0) and gm.prefill_route(2, 200) == (0, 0)
    assert gm.prefill_route(3, 200) == (3, 1)
    assert gm.prefill_route(158 * 3, 1000) == (474, 3)
    gm.set_option(L.OPT_PREFILL_ATTN, 2)               # ring passes need the shared-tile attention
    assert gm.prefill_route(400, 0) == (0, 0) and gm.prefill_route(100, 0) == (100, 1)
    gm.set_option(L.OPT_PREFILL_ATTN, 1)
    for bad in (-1, 2):
        with pytest.raises(L.XhError):
            gm.set_option(L.OPT_PREFILL_RING, bad)
    assert gm.get_option(L.OPT_PREFILL_RING) == 1
    gm.set_option(L.OPT_PREFILL_RING, 0)
    assert gm.get_option(L.OPT_PREFILL_RING) == 0
    assert gm.prefill_route(400, 0) == (0, 0) and gm.prefill_route(100, 200) == (0, 0)
    assert gm.prefill_route(100, 0) == (100, 1)
    gm.set_option(L.OPT_PREFILL, 0)
    assert gm.prefill_route(100, 0) == (0, 0)
    gm.close()


# 2, 7 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("wdt,passes", [(L.F16, 3), (L.BF16, 7)])
def test_laps(wdt, passes):
    """L = 160 (L - 2 = 158: no multiple of a tile): one prefill of 400 tokens from pos 0 crosses L
    and laps the ring more than twice, f16 in ring passes of 158 + 82, bf16 (the f32-input GEMM's
    64-token passes) in 64 + 64 + 64 + 48.  Last logits, every ring row of both layers, and — the
    step parameters the prompt leaves — 6 device greedy steps against the oracle."""
    msl, n = 160, 400
    c = base_cfg(msl)
    gm, om = build_pair(c, wdt)
    assert gm.prefill_route(n, 0) == (n, passes)
    toks = tokens(n)
    st = InferenceState(c)
    gm.prefill(toks, 0, st)
    ref = oracle_loop(om, toks, 0)
    check_logits(st.logits(), ref)
    check_rows(gm, om, c, [(0, msl)])
    nxt = gm.decode_greedy(n, 6)
    assert len(nxt) == 6
    check_teacher_forced(gm, om, nxt, n, st)
    gm.close()
    om.close()


# 3 ------------------------------------------------------------------------------------------
def test_full_length_pass():
    """The ring hydrated to pos 160, then one ring pass of exactly L - 2 = 158 tokens: its last
    row sees no history at all (every slot behind the sinks is the pass's own), its first rows
    nearly all of it."""
    msl = 160
    c = base_cfg(msl)
    gm, om = build_pair(c, L.F16)
    toks = tokens(msl + 158, mul=41)
    st = InferenceState(c)
    gm.prefill(toks[:msl], 0, st)
    assert gm.prefill_route(158, msl) == (158, 1)
    gm.prefill(toks[msl:], msl, st)
    ref = oracle_loop(om, toks, 0)
    check_logits(st.logits(), ref)
    check_rows(gm, om, c, [(0, msl)])
    gm.close()
    om.close()


# 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 256])
def test_wrap_inside_the_pass_with_splits(n):
    """32 q heads, 8 KV heads, L = 32768, the ring full of synthetic K/V, pos0 with kv_pos(pos0) =
    L - 10: the pass overwrites slots L-10 .. L-1, 2 .., across the physical wrap, and with
    XH_OPT_PREFILL_ATTN_SPLIT 1 its 8 ceil(n / 32) workgroups walk the window in up to 64 splits.
    Both forms against the oracle (logits, the written rows, both sink rows); the split form
    twice from the same ring, bit for bit.  The sink rows are an fp16-rounded iteration, so the
    device's contracted arithmetic and the oracle's plain C drift apart by a random walk: after
    these 256 tokens up to 0.0059 against the bar's 0.0062, on the token loop just the same."""
    msl = 32768
    c = make_cfg(256, 512, 2, 32, 8, 128, 512, msl)
    gm, om = build_pair(c, L.F16)
    pos0 = 2 * msl - 12
    assert kv_pos(pos0, msl) == msl - 10
    toks = [3 + (i * 31) % 500 for i in range(n)]
    fill(gm, om, c, msl, 3500)
    ref = oracle_loop(om, toks, pos0)
    assert gm.prefill_route(n, pos0) == (n, 1)
    st = InferenceState(c)
    got = {}
    for split in (1, 0, 1):
        fill(gm, None, c, msl, 3500)  # the pass before overwrote rows and rotated the sinks
        gm.set_option(L.OPT_PREFILL_ATTN_SPLIT, split)
        gm.prefill(toks, pos0, st)
        lg = st.logits().copy()
        check_logits(lg, ref, split)
        check_rows(gm, om, c, [(0, 2), (msl - 10, 10), (2, n - 10)], split)
        # the first history row the pass did not reach is as filled
        assert np.array_equal(gm.kv_read(0, 0, 2 + n - 10, 4), om.kv(0, 0)[2 + n - 10:6 + n - 10])
        if split in got:
            assert np.array_equal(lg.view(np.uint32), got[split].view(np.uint32))
        got[split] = lg
    gm.close()
    om.close()


# 5 ------------------------------------------------------------------------------------------
def test_sinks_bit_exact_against_the_token_loop():
    """From one full synthetic ring (L = 4096), 300 tokens at pos0 5000 as ring passes and, on a
    second context, through the token loop (XH_OPT_PREFILL_RING 0): the sink K rows of every layer
    are the same function iterated 300 times on the same bits — bit-identical, and not the rows
    they started from; every ring row the pass does not map to is still the fill, bit for bit."""
    msl, pos0, n = 4096, 5000, 300
    c = base_cfg(msl)
    toks = tokens(n, mul=43)
    rows = {}
    for ring in (1, 0):
        gm, om = build_pair(c, L.F16)
        om.close()
        fill(gm, None, c, msl, 3700)
        start = [gm.kv_read(layer, 0, 0, 2) for layer in range(c.n_layers)]
        gm.set_option(L.OPT_PREFILL_RING, ring)
        assert gm.prefill_route(n, pos0) == ((n, 1) if ring else (0, 0))
        gm.prefill(toks, pos0)
        rows[ring] = [[gm.kv_read(layer, which, 0, msl) for which in (0, 1)] for layer in range(c.n_layers)]
        for layer in range(c.n_layers):
            assert not np.array_equal(rows[ring][layer][0][:2], start[layer])
        gm.close()
    s0 = kv_pos(pos0, msl)
    assert s0 + n <= msl  # the mapped rows are s0 .. s0 + n - 1
    kv_dim = c.n_kv_heads * c.head_dim
    for layer in range(c.n_layers):
        assert np.array_equal(rows[1][layer][0][:2], rows[0][layer][0][:2]), layer
        for which in (0, 1):
            filled = O.synthetic(msl, kv_dim, L.F16, 3700 + 2 * layer + which, 0.0, 1.0)
            lo = 2 if which == 0 else 0  # V's sink rows are never written
            for got in (rows[1][layer][which], rows[0][layer][which]):
                assert np.array_equal(got[lo:s0], filled[lo:s0]), (layer, which)
                assert np.array_equal(got[s0 + n:], filled[s0 + n:]), (layer, which)
            # the mapped rows agree between the routes within the K/V bar
            a, b = f16(rows[1][layer][which][s0:s0 + n]), f16(rows[0][layer][which][s0:s0 + n])
            assert np.abs(a - b).max() <= 2e-3 * max(1.0, float(np.abs(b).max())), (layer, which)


# 6 ------------------------------------------------------------------------------------------
def test_crossing_with_a_long_history():
    """L = 4096 with a synthetic history in slots 0 .. 3995: one prefill of 600 tokens at pos0 3996
    runs 100 tokens inside the ring, then 500 as a ring pass over that history."""
    msl, hist, n = 4096, 3996, 600
    c = base_cfg(msl)
    gm, om = build_pair(c, L.F16)
    fill(gm, om, c, hist, 3900)
    toks = tokens(n, mul=47)
    assert gm.prefill_route(n, hist) == (n, 2)
    st = InferenceState(c)
    gm.prefill(toks, hist, st)
    ref = oracle_loop(om, toks, hist)
    check_logits(st.logits(), ref)
    check_rows(gm, om, c, [(0, 2), (hist, msl - hist), (2, 500)])
    assert np.array_equal(gm.kv_read(1, 1, 502, 8), om.kv(1, 1)[502:510])
    gm.close()
    om.close()


# 8 ------------------------------------------------------------------------------------------
def test_perplexity_across_the_wrap():
    """token_probs over 400 tokens at L = 160 (399 forwarded: 160 inside the ring, 158 + 81 as ring
    passes) against Sampler::sample_prob of the oracle's token loop, with ring passes and with the
    token loop (XH_OPT_PREFILL_RING 0)."""
    msl, n = 160, 400
    c = base_cfg(msl)
    gm, om = build_pair(c, L.F16)
    toks = tokens(n, mul=53)
    refs = []
    for pos in range(n - 1):
        om.forward(toks[pos], pos)
        lg = om.logits().copy()
        refs.append((lg, O.sample_prob(lg, toks[pos + 1])))
    for ring in (1, 0):
        gm.reset()
        gm.set_option(L.OPT_PREFILL_RING, ring)
        got = gm.token_probs(toks)
        assert got.shape == (n - 1,)
        for pos, (lg, ref) in enumerate(refs):
            if ref < 1e-30:
                assert got[pos] < 1e-30, (ring, pos, got[pos], ref)
                continue
            assert got[pos] > 0, (ring, pos, got[pos], ref)
            check_logp(float(abs(np.log(got[pos]) - np.log(ref))), lg, None, (ring, pos))
    gm.close()
    om.close()


# 9 ------------------------------------------------------------------------------------------
def test_other_head_shapes_keep_the_token_loop():
    """tiny_mistral has head_dim 16: with -T 16 a 41-token prompt routes nothing to passes and
    still matches the oracle."""
    xf = XalmFile(fixture_path("tiny_mistral_f16.xalm"))
    gm = Model.from_xalm(xf, context=16)
    om = O.OracleModel.from_xalm(xf, context=16)
    toks = [1] + [3 + (i * 23) % 290 for i in range(40)]
    assert gm.get_option(L.OPT_PREFILL_RING) == 1
    assert gm.prefill_route(len(toks), 0) == (0, 0)
    st = InferenceState(gm.config)
    gm.prefill(toks, 0, st)
    ref = oracle_loop(om, toks, 0)
    check_logits(st.logits(), ref)
    gm.close()
    om.close()
