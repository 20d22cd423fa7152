"""The decode-attention regime sweep on the CPU: the case table against the code's own plan, the
bar against the f32 oracle, and the planted probes' precondition (tests/attn_cases.py, attn_ref.py)."""
import numpy as np
import pytest

from oracle import oracle as O
from xalm_amd import _lib as L

import attn_cases as AC
import attn_ref as AR
import kv8_ref

ROW_IDS = [AC.row_id(r) for r in AC.ROWS]
PLAN_FIELDS = [n for n, _ in L.XhAttnPlan._fields_]


def test_plan_is_declared_and_checks_its_arguments():
    p = L.attn_plan(128, 32, 8, 4096, L.F16, 1, 4096)  # Mistral's head shape, 4k: 16 splits of 256, merged on arrival
    assert {n: getattr(p, n) for n in PLAN_FIELDS} == dict(fused=1, nsplit=16, T=256, n_active=16, step=128, rounds_full=2,
                                                           rounds_last=2, wph=4, merge_mb=8, merge_nc=1, stage=5)
    assert L.attn_plan(128, 32, 8, 4096, L.F16, 1, 128).stage == 1
    for bad in ((128, 32, 8, 4096, L.F8_E4M3, 1, 10),  # no fused launch on the fp8 ring
                (64, 8, 4, 4096, L.F16, 1, 10),         # 64 x 2: not instantiated
                (128, 32, 8, 4096, L.F16, 0, 4097), (128, 32, 8, 4096, L.F16, 0, 0), (48, 4, 1, 64, L.F16, 0, 1),
                (128, 3, 1, 64, L.F16, 0, 1), (128, 4, 1, 64, L.BF16, 0, 1)):
        with pytest.raises(L.XhError):
            L.attn_plan(*bad)


def test_the_defect_regime_takes_two_loads_per_lane():
    """Past 64 active splits a lane must load two (m, l) pairs, whatever the chunk per merge group."""
    for r in AC.ROWS:
        for kv_len in range(1, r.msl + 1):
            p = AC.plan(r, kv_len)
            assert p.n_active <= 64 * max(1, p.merge_nc) or p.merge_mb == 0, (AC.row_id(r), kv_len, p.n_active, p.merge_mb)
    p = AC.plan(AC.Row(0, L.F16, 16, 1, 1, 16640), 16640)
    assert (p.nsplit, p.T, p.n_active, p.merge_mb, p.merge_nc) == (65, 256, 65, 16, 2)


@pytest.mark.parametrize("r", AC.ROWS, ids=ROW_IDS)
def test_table_holds_first_and_last_kv_len_of_every_regime(r):
    have = set(AC.LENS[AC.row_id(r)])
    missing = {reg: [k for k in fl if k not in have] for reg, fl in AC.reachable(r).items()}
    missing = {reg: ks for reg, ks in missing.items() if ks}
    for reg, ks in sorted(missing.items()):
        print(f"{AC.row_id(r)}: regime ({AC.REGIME_FIELDS}) = {reg} lacks kv_len {ks}")
    assert not missing, missing
    assert all(1 <= k <= r.msl for k in AC.lens(r))


def test_rows_are_the_issues():
    split = {(r.head_dim, r.qpk) for r in AC.ROWS if not r.fused}
    assert split == {(128, 4), (128, 8), (128, 1), (64, 1), (64, 4), (32, 2), (16, 1), (16, 2), (16, 4), (256, 8)}
    assert {(r.head_dim, r.qpk) for r in AC.ROWS if r.fused} == {(128, 4), (128, 8), (64, 4), (16, 2)}
    assert all(r.msl <= (8192 if r.fused else 32768) and r.msl * r.n_kv * r.head_dim <= 32768 * 128 for r in AC.ROWS)
    for dt in (L.F16, L.F8_E4M3):
        assert 16640 in AC.lens(AC.Row(0, dt, 16, 1, 1, 16640)) and 20000 in AC.lens(AC.Row(0, dt, 64, 1, 1, 32768))
        assert any(AC.plan(r, k).n_active == 128 for r in AC.ROWS if r.kv_dtype == dt and not r.fused for k in AC.lens(r)[-1:])
    for r in AC.ROWS:
        if r.fused:  # every stage form, and every split active at the end (16 x 2: its floor of 1024
            # slots keeps a ring of 8192 at 8 active splits of the grid's 32)
            assert {AC.plan(r, k).stage for k in AC.lens(r)} == {1, 2, 3, 4, 5}
            p = AC.plan(r, r.msl)
            assert p.n_active == (p.nsplit if r.head_dim != 16 else 8)


def oracle_mha(r, kb, vb, q, kv_len):
    img = lambda a: kv8_ref.image16(a) if r.kv_dtype == L.F8_E4M3 else a
    return O.mha(img(kb), img(vb), q, r.head_dim, kv_len, r.msl, r.n_kv * r.qpk, r.n_kv)


@pytest.mark.parametrize("r", AC.ROWS, ids=ROW_IDS)
def test_oracle_has_4x_headroom_under_the_bar(r):
    kb, vb, q = AR.inputs(r)
    k64, v64 = AR.decode_ring(kb, r.kv_dtype), AR.decode_ring(vb, r.kv_dtype)
    worst = (-1.0, 0)
    for kv_len in AC.lens(r):
        att, bar, _ = AR.attention64(k64, v64, q, r.head_dim, kv_len, r.n_kv * r.qpk, r.n_kv)
        ratio = float(np.max(np.abs(oracle_mha(r, kb, vb, q, kv_len) - att) / bar))
        worst = max(worst, (ratio, kv_len))
    print(f"{AC.row_id(r)}: oracle worst err / bar {worst[0]:.3f} at kv_len {worst[1]}")
    assert worst[0] <= 0.25, worst


@pytest.mark.parametrize("r", AC.ROWS, ids=ROW_IDS)
def test_planted_probes_meet_their_precondition(r):
    """Every probe: in float64 every weight off the planted slot is below 2^-150 for the planted
    head and the f32 oracle returns V[t] itself for it.  The other heads of the group see one
    large score over thousands of small ones; the oracle adds its weights one by one in f32, where
    terms below half an ulp of the running sum are lost (sequential summation, error up to
    n 2^-24 sum|terms|), so its ratio for them is printed, not bounded: 1.47 at worst, 128 x 4 on the
    e4m3 ring at kv_len 32768.  The device sums a few terms per lane and then trees; it is held to
    the bar there (test_attn_regimes_gpu.py)."""
    kb0, vb, q = AR.inputs(r)
    v64 = AR.decode_ring(vb, r.kv_dtype)
    n_heads, hd = r.n_kv * r.qpk, r.head_dim
    worst, n = 0.0, 0
    for kv_len in AC.probe_lens(r):
        for i, t in enumerate(AC.probe_slots(r, kv_len)):
            kb, head = kb0.copy(), i % r.qpk
            AR.plant(kb, q, t, head, r.kv_dtype, hd, kv_len, n_heads, r.n_kv)
            att, bar, off = AR.attention64(AR.decode_ring(kb, r.kv_dtype), v64, q, hd, kv_len, n_heads, r.n_kv)
            got = oracle_mha(r, kb, vb, q, kv_len)
            for g in range(r.n_kv):
                h = g * r.qpk + head
                assert off[h] < 2.0 ** -150, (kv_len, t, h, off[h])
                assert AR.values_equal(got[h * hd:(h + 1) * hd], v64[t, g * hd:(g + 1) * hd]), (kv_len, t, h)
            others = np.ones(n_heads * hd, bool)
            for g in range(r.n_kv):
                others[(g * r.qpk + head) * hd:(g * r.qpk + head + 1) * hd] = False
            if others.any():
                worst = max(worst, float(np.max(np.abs(got - att)[others] / bar[others])))
            n += 1
    print(f"{AC.row_id(r)}: {n} probes, oracle worst err / bar off the planted heads {worst:.3f}")
