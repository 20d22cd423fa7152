"""Decode attention against float64 in every split and merge regime.

Split route: every case of tests/attn_cases.py's split rows through xh_op_mha / xh_op_mha8 against
tests/attn_ref.py at its bar; the planted-slot probes, exact for the planted head and at the bar
for the others; and one case per row twice, bit for bit.
Fused route: a one-layer model (hidden 64, vocab 64, W2 zero so that the residual stream read back
is x1 = x0 + Wo att, the method of test_stages_gpu.py) with the fused attention + Wo launch and with
the two launches, against x0 + Wo att in float64 from the observed q and the observed ring: every
case of the fused rows with F16 weights, the six fused Wo dtypes per stage form, the whole-row Wo
branch at 4096 inputs, planted probes through kv_write, graph replays across the stage boundaries,
the full ring with sinks, the fp8 ring, and the ticket counters of a context that is used again.
Each test prints its worst err / bar.
"""
import hashlib
import json

import numpy as np
import pytest

from conftest import fixture_path
from xalm_amd import _lib as L
from xalm_amd.model import Model

import attn_cases as AC
import attn_ref as AR
import stage_cases as SC
import stage_ref as SR

pytestmark = pytest.mark.gpu

SPLIT_ROWS = [r for r in AC.ROWS if not r.fused]
SPLIT_IDS = [AC.row_id(r) for r in SPLIT_ROWS]


def op_mha(r, kb, vb, q, kv_len):
    op = L.op_mha8 if r.kv_dtype == L.F8_E4M3 else L.op_mha
    return op(kb, vb, q, r.head_dim, kv_len, r.msl, r.n_kv * r.qpk, r.n_kv)


def describe(r, kv_len):
    p = AC.plan(r, kv_len)
    return f"kv_len {kv_len}: n_active {p.n_active}, T {p.T}, rounds {p.rounds_full}/{p.rounds_last}, merge {p.merge_mb}x{p.merge_nc}"


@pytest.mark.parametrize("r", SPLIT_ROWS, ids=SPLIT_IDS)
def test_split_route_every_case_against_float64(r):
    kb, vb, q = AR.inputs(r)
    k64, v64 = AR.decode_ring(kb, r.kv_dtype), AR.decode_ring(vb, r.kv_dtype)
    bad, worst = [], (-1.0, 0)
    for kv_len in AC.lens(r):
        att, bar, _ = AR.attention64(k64, v64, q, r.head_dim, kv_len, r.n_kv * r.qpk, r.n_kv)
        got = op_mha(r, kb, vb, q, kv_len)
        err = np.abs(got - att)
        ratio = float(np.max(err / bar))
        worst = max(worst, (ratio, kv_len))
        if not ratio <= 1.0:
            bad.append(f"{describe(r, kv_len)}: err / bar {ratio:.3g}, err {float(err.max()):.3g}")
    print(f"{AC.row_id(r)}: {len(AC.lens(r))} cases, worst err / bar {worst[0]:.3f} at {describe(r, worst[1])}")
    assert not bad, bad


@pytest.mark.parametrize("r", SPLIT_ROWS, ids=SPLIT_IDS)
def test_split_route_planted_probes(r):
    kb0, vb, q = AR.inputs(r)
    v64 = AR.decode_ring(vb, r.kv_dtype)
    n_heads, hd = r.n_kv * r.qpk, r.head_dim
    bad, worst, n = [], 0.0, 0
    for kv_len in AC.probe_lens(r):
        for i, t in enumerate(AC.probe_slots(r, kv_len)):
            kb, head = kb0.copy(), i % r.qpk
            AR.plant(kb, q, t, head, r.kv_dtype, hd, kv_len, n_heads, r.n_kv)
            att, bar, _ = AR.attention64(AR.decode_ring(kb, r.kv_dtype), v64, q, hd, kv_len, n_heads, r.n_kv)
            got = op_mha(r, kb, vb, q, kv_len)
            others = np.ones(n_heads * hd, bool)
            for g in range(r.n_kv):
                hs = slice((g * r.qpk + head) * hd, (g * r.qpk + head + 1) * hd)
                others[hs] = False
                if not AR.values_equal(got[hs], v64[t, g * hd:(g + 1) * hd]):
                    bad.append(f"{describe(r, kv_len)}: slot {t}, head {g * r.qpk + head} is not V[t]: off by "
                               f"{float(np.abs(got[hs] - v64[t, g * hd:(g + 1) * hd]).max()):.3g}")
            if others.any():
                ratio = float(np.max(np.abs(got - att)[others] / bar[others]))
                worst = max(worst, ratio)
                if not ratio <= 1.0:
                    bad.append(f"{describe(r, kv_len)}: slot {t}, heads off the plant err / bar {ratio:.3g}")
            n += 1
    print(f"{AC.row_id(r)}: {n} probes, worst err / bar off the planted heads {worst:.3f}")
    assert not bad, bad


@pytest.mark.parametrize("r", SPLIT_ROWS, ids=SPLIT_IDS)
def test_split_route_repeats_bit_for_bit(r):
    """The row's longest case twice: the merge's order is fixed (group sums in group order), so the
    outputs repeat bit for bit whichever split arrives last.  (xh_op_mha allocates its ticket
    counters per call; their restoration is test_ticket_counters_are_restored's, on one context.)"""
    kb, vb, q = AR.inputs(r)
    kv_len = AC.lens(r)[-1]
    a, b = op_mha(r, kb, vb, q, kv_len), op_mha(r, kb, vb, q, kv_len)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), describe(r, kv_len)


def test_split_route_outputs_up_to_64_splits_are_the_recorded_ones():
    """tests/golden/attn_split_outputs_hash.json holds, for every split-route case of up to 64
    active splits (660; the cases above 64 are not recorded: the build before the fix had them
    wrong), the first 24 hex digits of the SHA-256 of its output as the build before the merge fix
    gave it.  The fix touches only steps with more than 64 active splits, and lifting the launch
    geometry into constexpr functions touches none: every recorded case is bit for bit what it
    was.  (A change that means to move these bits records the file again.)"""
    with open(fixture_path("attn_split_outputs_hash.json")) as f:
        want = json.load(f)
    assert len(want) == 660
    diff, n = [], 0
    for r in SPLIT_ROWS:
        kb, vb, q = AR.inputs(r)
        for kv_len in AC.lens(r):
            if AC.plan(r, kv_len).n_active > 64:
                continue
            got = hashlib.sha256(np.ascontiguousarray(op_mha(r, kb, vb, q, kv_len)).tobytes()).hexdigest()[:24]
            n += 1
            if got != want[f"{AC.row_id(r)}@{kv_len}"]:
                diff.append(f"{AC.row_id(r)}@{kv_len}")
    print(f"{n} cases compared")
    assert n == 660 and not diff, diff


# ---- the fused route, in the model -----------------------------------------------------------------
FUSED_ROWS = [r for r in AC.ROWS if r.fused]
FUSED_IDS = [AC.row_id(r) for r in FUSED_ROWS]
M128 = AC.Row(1, L.F16, 128, 4, 1, 2048)
WO_DTYPES = (L.F32, L.F16, L.BF16, L.F8_E4M3, L.F8_E5M2, L.Q8)


class Ctx:
    """A one-layer model of a row's head shape: weights of dtype wdt, W2 zero, the ring full of
    synthetic history; steps that return what they left, and the float64 x1 of a step."""

    def __init__(self, r, wdt=L.F16, dim=64, kv_dtype=L.F16, expect_fused=True):
        self.r, self.kv_dtype = r, kv_dtype
        self.c = c = SC.case(dim, 64, heads=r.qpk * r.n_kv, kv_heads=r.n_kv, head_dim=r.head_dim, dtypes=(wdt,))
        cfg = SC.config(c)
        cfg.max_seq_len = r.msl
        self.gm = gm = Model(cfg, kv_dtype=kv_dtype)
        W = SR.host_weights(c, wdt)
        for kind, dt, seed, mean, std in SR.tensor_specs(c, wdt):
            if kind == L.W2:
                gm.upload(kind, 0, dt, SR.zero_matrix(dt, c.dim, c.hidden))
            elif dt == L.Q8:
                gm.upload(kind, 0, dt, W[kind][1])
            else:
                gm.upload_synthetic(kind, 0, dt, seed, mean, std)
        for which in (0, 1):
            gm.kv_fill_synthetic(0, which, 0, r.msl, SR.KV_SEED[which], 1.0)
        self.wo, self.wom = SR.decode64(W[L.WO][0], W[L.WO][1], c.heads * c.head_dim)
        edt, emb = W[L.EMBED]
        self.x0 = SR.decode64(edt, emb[SC.TOKEN:SC.TOKEN + 1], c.dim)[0][0]
        self.check_route(expect_fused)

    def check_route(self, expect_fused):
        """OPT_FUSE_ATTN_WO 1 takes the fused launch (its workgroups stamp the trace) where one is
        expected, and 0 never does."""
        gm = self.gm
        gm.debug_trace(2)
        for fuse, want in ((1, expect_fused), (0, False)):
            gm.set_option(L.OPT_FUSE_ATTN_WO, fuse)
            gm.forward(None, SC.TOKEN, 0, L.HYDRATE_KV_CACHE)
            gm.debug_read(L.READ_X)  # waits for the step
            assert bool(gm.debug_trace(2).any()) == want, (AC.row_id(self.r), fuse, want)
        gm.debug_trace(0)
        for which in (0, 1):  # slot 0 as the history had it
            gm.kv_fill_synthetic(0, which, 0, 1, SR.KV_SEED[which], 1.0)

    def ring(self, kv_len):
        read = self.gm.kv_read8 if self.kv_dtype == L.F8_E4M3 else self.gm.kv_read
        return tuple(read(0, which, 0, kv_len) for which in (0, 1))

    def step(self, pos, fuse):
        """(x1, q, kb, vb, kv_len) of one step at pos."""
        if self.gm.get_option(L.OPT_FUSE_ATTN_WO) != fuse:  # setting it drops the captured graphs
            self.gm.set_option(L.OPT_FUSE_ATTN_WO, fuse)
        self.gm.forward(None, SC.TOKEN, pos, L.HYDRATE_KV_CACHE)
        kv_len = min(pos + 1, self.r.msl)
        return (self.gm.debug_read(L.READ_X), self.gm.debug_read(L.READ_Q)) + self.ring(kv_len) + (kv_len,)

    def reference(self, q, kb, vb, kv_len, exact=None):
        """(x1, bar): x0 + Wo att in float64; bar 2e-6 mag + 1e-7 + |Wo| @ bar_att.  exact = (head,
        values): that head's attention output is these values, with no attention term in the bar."""
        c = self.c
        att, bar_att, _ = AR.attention64(AR.decode_ring(kb, self.kv_dtype), AR.decode_ring(vb, self.kv_dtype), q,
                                         c.head_dim, kv_len, c.heads, c.kv_heads)
        if exact is not None:
            hs = slice(exact[0] * c.head_dim, (exact[0] + 1) * c.head_dim)
            att[hs], bar_att[hs] = exact[1], 0.0
        x1, b = SR.matvec(self.wo, self.wom, att, self.x0)
        return x1, b + self.wom @ bar_att

    def ratio(self, pos, fuse):
        x1, q, kb, vb, kv_len = self.step(pos, fuse)
        ref, bar = self.reference(q, kb, vb, kv_len)
        return float(np.max(np.abs(x1 - ref) / bar))

    def close(self):
        self.gm.close()


def stage_lens(r):
    """{stage form: the last kv_len of the row's table that takes it}."""
    return {AC.plan(r, k).stage: k for k in AC.lens(r)}


def run_cases(m, cases, label):
    """cases: [(name, pos, fuse)]; every step against float64 at the bar."""
    bad, worst = [], (-1.0, "")
    for name, pos, fuse in cases:
        ratio = m.ratio(pos, fuse)
        worst = max(worst, (ratio, name))
        if not ratio <= 1.0:
            bad.append(f"{name}: err / bar {ratio:.3g}")
    print(f"{label}: {len(cases)} steps, worst err / bar {worst[0]:.3f} at {worst[1]}")
    assert not bad, bad


@pytest.mark.parametrize("r", FUSED_ROWS, ids=FUSED_IDS)
def test_fused_route_every_case_against_float64(r):
    m = Ctx(r)
    try:
        cases = []
        for kv_len in AC.lens(r):
            p = AC.plan(r, kv_len)
            cases += [(f"fuse {fuse}, kv_len {kv_len} (n_active {p.n_active}, stage {p.stage})", kv_len - 1, fuse)
                      for fuse in (1, 0)]
        run_cases(m, cases, AC.row_id(r))
    finally:
        m.close()


@pytest.mark.parametrize("wdt", WO_DTYPES, ids=[SC.DT_NAME[d] for d in WO_DTYPES])
def test_fused_route_every_wo_dtype_at_every_stage_form(wdt):
    m = Ctx(M128, wdt)
    try:
        run_cases(m, [(f"fuse {fuse}, stage {st}, kv_len {k}", k - 1, fuse) for st, k in sorted(stage_lens(M128).items())
                      for fuse in (1, 0)], f"{AC.row_id(M128)} {SC.DT_NAME[wdt]}")
    finally:
        m.close()


@pytest.mark.parametrize("wdt", [L.F16, L.F8_E4M3], ids=["F16", "F8_E4M3"])
def test_fused_route_whole_row_wo_at_4096_inputs(wdt):
    """32 x 128 heads over 8 KV heads, dim 4096: a Wo row is exactly the U chunks a wave requests
    before the hand-off (ga.n == U * 64 * E), the branch no small shape takes.  Stage forms 1 and 5."""
    r = AC.Row(1, L.F16, 128, 4, 8, 2048)
    st = {AC.plan(r, k).stage: k for k in (100, 2048)}
    assert set(st) == {1, 5}
    m = Ctx(r, wdt, dim=4096)
    try:
        run_cases(m, [(f"fuse {fuse}, stage {s}, kv_len {k}", k - 1, fuse) for s, k in sorted(st.items()) for fuse in (1, 0)],
                  f"{AC.row_id(r)} dim 4096 {SC.DT_NAME[wdt]}")
    finally:
        m.close()


@pytest.mark.parametrize("r", FUSED_ROWS, ids=FUSED_IDS)
def test_fused_route_planted_probes(r):
    """A first step yields q and the ring; the planted K row goes in with kv_write; the second step
    has the same q bit for bit, and x1 is x0 + Wo att with the planted head's att = V[t] exactly (no
    attention term for its columns of Wo).  Slot kv_len - 1 is the step's own row, so it is not planted."""
    m = Ctx(r)
    hd = r.head_dim
    try:
        bad, worst, n = [], 0.0, 0
        for kv_len in AC.probe_lens(r):
            for i, t in enumerate(s for s in AC.probe_slots(r, kv_len) if s != kv_len - 1):
                head = i % r.qpk
                for fuse in (1, 0):
                    _, q, kb, vb, _ = m.step(kv_len - 1, fuse)
                    kb = kb.copy()
                    AR.plant(kb, q, t, head, L.F16, hd, kv_len, m.c.heads, m.c.kv_heads)
                    m.gm.kv_write(0, 0, t, kb[t:t + 1])
                    x1, q2, kb2, vb2, _ = m.step(kv_len - 1, fuse)
                    assert np.array_equal(q.view(np.uint32), q2.view(np.uint32)) and np.array_equal(kb, kb2)
                    ref, bar = m.reference(q2, kb2, vb2, kv_len, exact=(head, AR.decode_ring(vb2[t, :hd], L.F16)))
                    ratio = float(np.max(np.abs(x1 - ref) / bar))
                    worst, n = max(worst, ratio), n + 1
                    if not ratio <= 1.0:
                        bad.append(f"fuse {fuse}, kv_len {kv_len}, slot {t}, head {head}: err / bar {ratio:.3g}")
                    m.gm.kv_fill_synthetic(0, 0, t, 1, SR.KV_SEED[0] + 7919 * (t + 1), 1.0)  # an ordinary row again
        print(f"{AC.row_id(r)}: {n} probes, worst err / bar {worst:.3f}")
        assert not bad, bad
    finally:
        m.close()


def test_fused_route_graph_replays_across_stage_boundaries():
    """One captured graph replayed across the first kv_len of stage forms 2 and 5.  The fuse option is
    set once and the graphs switched on once, both before the first step (either call drops the
    captured graphs); after that the test only calls forward, debug_read and kv_read, none of which
    drops them, so the step at kv_len b - 2 captures the graph and the four steps after it replay
    it.  Between two replays the hand-off target goes from n_kv * n_active to n_kv and the stage form
    changes, all from the kv_len the device reads, and each launch's sync words are reset by the
    next.  Then the same with graphs off (every launch enqueued afresh): x1 bit for bit the same."""
    m = Ctx(M128)
    gm = m.gm
    try:
        first = {}
        for k in range(1, M128.msl + 1):
            first.setdefault(AC.plan(M128, k).stage, k)
        lens = []
        for st in (2, 5):
            b = first[st]
            assert AC.plan(M128, b - 1).stage == st - 1 and AC.plan(M128, b).n_active == AC.plan(M128, b - 1).n_active + 1
            lens += list(range(b - 2, b + 3))
        seen = {}
        for graphs in (True, False):
            gm.set_option(L.OPT_FUSE_ATTN_WO, 1)
            gm.set_graphs(graphs)
            bad, worst = [], (-1.0, 0)
            for kv_len in lens:  # nothing below drops a captured graph
                gm.forward(None, SC.TOKEN, kv_len - 1, L.HYDRATE_KV_CACHE)
                x1, q = gm.debug_read(L.READ_X), gm.debug_read(L.READ_Q)
                kb, vb = m.ring(kv_len)
                ref, bar = m.reference(q, kb, vb, kv_len)
                ratio = float(np.max(np.abs(x1 - ref) / bar))
                worst = max(worst, (ratio, kv_len))
                if not ratio <= 1.0:
                    bad.append(f"graphs {graphs}, kv_len {kv_len} (stage {AC.plan(M128, kv_len).stage}): err / bar {ratio:.3g}")
                if graphs:
                    seen[kv_len] = x1
                else:
                    assert np.array_equal(seen[kv_len].view(np.uint32), x1.view(np.uint32)), kv_len
            print(f"{AC.row_id(M128)} graphs {graphs}: {len(lens)} steps, worst err / bar {worst[0]:.3f} at kv_len {worst[1]}")
            assert not bad, bad
    finally:
        m.close()


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "two-launches"])
def test_ring_full_with_sinks(fuse):
    """pos = max_seq_len + 3: kv_len is the whole ring, the step's row goes to slot 5 behind the two sinks."""
    m = Ctx(M128)
    try:
        run_cases(m, [(f"pos {M128.msl + 3}", M128.msl + 3, fuse)], f"{AC.row_id(M128)} ring full, fuse {fuse}")
    finally:
        m.close()


@pytest.mark.parametrize("qpk", [2, 4, 8])
def test_fp8_ring_in_the_model(qpk):
    """One case per attn_kv_elems form (16, 8, 4 elements per lane) at two active splits, from the
    observed codes (kv_read8).  The fp8 ring has no fused launch: both settings take two launches."""
    r = AC.Row(0, L.F8_E4M3, 128, qpk, 1, 512)
    assert AC.plan(r, 300).n_active == 2
    m = Ctx(r, kv_dtype=L.F8_E4M3, expect_fused=False)
    try:
        run_cases(m, [(f"kv_len 300, fuse {fuse}", 299, fuse) for fuse in (1, 0)], AC.row_id(r))
    finally:
        m.close()


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "two-launches"])
def test_ticket_counters_are_restored(fuse):
    """Steps A, B, A on one context, every split active and the last one to arrive merging (stage
    form 5 when fused): were a head's ticket counter not put back to zero, no later block would draw
    the last ticket, nothing would merge, and the output would stay the step before's.  Each step is
    held to the bar, and the second A repeats the first bit for bit (B writes a slot past A's)."""
    m = Ctx(M128)
    try:
        a, b = M128.msl - 300, M128.msl
        assert AC.plan(M128, a).n_active > 4 and AC.plan(M128, b).n_active > 4
        xa, q, kb, vb, _ = m.step(a - 1, fuse)
        ref, bar = m.reference(q, kb, vb, a)
        assert np.max(np.abs(xa - ref) / bar) <= 1.0
        assert m.ratio(b - 1, fuse) <= 1.0
        xa2 = m.step(a - 1, fuse)[0]
        assert np.array_equal(xa.view(np.uint32), xa2.view(np.uint32))
        assert not np.array_equal(xa, m.step(b - 1, fuse)[0])
    finally:
        m.close()
