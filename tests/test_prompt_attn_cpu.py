"""The prompt attention's bar (tests/prompt_attn_ref.py) against its own conditions, on the CPU, over
the whole case table of tests/test_prompt_attn_gpu.py:
  (a) a correct f32 evaluation in another summation order stays within bar / 4: the oracle's mha
      row by row for the causal cases, a plain float32 numpy evaluation for the ring;
  (b) where some row sees 2 .. 64 walked keys, an evaluation that drops the lo half of q, or of p,
      exceeds the bar at its worst element by at least 2x.  (One key alone has p = 1 and out = V
      exactly under either mutant, so n = 1 at pos0 = 0 cannot tell them apart and is left to (a);
      a ring row always sees its whole window, so the short-window cases are those with W <= 64.)
The measured ratios are printed (-s) and recorded in DESIGN.md section 3.
"""
import numpy as np
import pytest

from oracle import oracle as O

import prompt_attn_ref as R

CASES = R.CAUSAL_CASES + R.RING_CASES
DISTINCT = list({R.input_key(c): c for c in CASES}.values())  # mode / nsplit do not change the inputs


def test_case_table_is_the_issue_s():
    assert len(set(CASES)) == len(CASES)
    groups = {g: sum(c.group == g for c in CASES) for g in {c.group for c in CASES}}
    assert groups == {"heads": 28, "edges": 31, "splits": 28, "peaked": 4, "ring": 36, "ring-splits": 6}, groups
    assert max(c.n for c in R.CAUSAL_CASES) <= 300 and max(c.m for c in R.RING_CASES) <= 200  # small shapes


def f32_oracle(c):
    if isinstance(c, R.Ring):
        return R.variant(c, "f32")
    q, k, v = R.inputs(c)
    S = c.pos0 + c.n
    return np.stack([O.mha(k, v, q[t], c.hd, c.pos0 + t + 1, S, c.n_heads, c.n_kv) for t in range(c.n)])


@pytest.mark.parametrize("c", DISTINCT, ids=R.case_id)
def test_f32_evaluation_is_within_a_quarter_of_the_bar(c):
    r = R.ratio(f32_oracle(c), c)
    print(f"\n{R.case_id(c)}: f32 / bar = {r:.4f}")
    assert r <= 0.25, r


def short_window(c):
    rows = c.n if isinstance(c, R.Causal) else c.m
    return R.fewest_keys(c) <= 64 and not (isinstance(c, R.Causal) and c.pos0 + rows < 2)


@pytest.mark.parametrize("c", [c for c in DISTINCT if short_window(c)], ids=R.case_id)
def test_mutants_exceed_the_bar_on_short_windows(c):
    rq, rp = R.ratio(R.variant(c, "q_hi_only"), c), R.ratio(R.variant(c, "p_hi_only"), c)
    print(f"\n{R.case_id(c)}: q_hi_only / bar = {rq:.2f}, p_hi_only / bar = {rp:.2f}")
    assert rq >= 2.0 and rp >= 2.0, (rq, rp)


def test_reference_against_the_definition_spelt_out():
    """The vectorised reference against scalar loops over the definition: one causal and one ring
    case, three rows each (first, a middle one, last), every head."""
    c = R.Causal("", 8, 4, 64, 7, 5, 0, 0, "rand")
    q, k, v = R.inputs(c)
    ref, _ = R.reference(c)
    K, V = R.f16_vals(k).reshape(-1, 4, 64), R.f16_vals(v).reshape(-1, 4, 64)
    sc = float(R.attn_scale(64))
    for t in (0, 3, 6):
        for h in range(8):
            g, qh = h // 2, q[t].astype(np.float64)[h * 64:(h + 1) * 64]
            s = np.array([qh @ K[j, g] * sc for j in range(c.pos0 + t + 1)])
            p = np.exp(s - s.max())
            want = sum(p[j] * V[j, g] for j in range(s.size)) / p.sum()
            assert np.allclose(ref[t, h * 64:(h + 1) * 64], want, rtol=1e-12, atol=1e-14)
    r = R.Ring("", 8, 2, 10, 10 + 13, 5, 0)  # W = 8: a window that wraps from slot 9 to slot 2
    q, kr, vr, ks, vs, sv = R.inputs(r)
    ref, _ = R.reference(r)
    W, hoff = 8, (r.p0 - 2) % 8
    f = lambda a: R.f16_vals(a).reshape(a.shape[:-1] + (2, 128))
    kr_, vr_, ks_, vs_, sv_ = f(kr), f(vr), f(ks), f(vs), f(sv)
    sc = float(R.attn_scale(128))
    for t in (0, 2, 4):
        for h in range(8):
            g, qh = h // 4, q[t].astype(np.float64)[h * 128:(h + 1) * 128]
            keys = [(sv_[t, 0, g], vr_[0, g]), (sv_[t, 1, g], vr_[1, g])]
            for u in range(t + 1, W + t + 1):
                keys.append((kr_[2 + (hoff + u) % W, g], vr_[2 + (hoff + u) % W, g]) if u < W else (ks_[u - W, g], vs_[u - W, g]))
            s = np.array([qh @ kk * sc for kk, _ in keys])
            p = np.exp(s - s.max())
            want = sum(pj * vv for pj, (_, vv) in zip(p, keys)) / p.sum()
            assert np.allclose(ref[t, h * 128:(h + 1) * 128], want, rtol=1e-12, atol=1e-14)


def test_ring_after_commit_moves_rows_exactly():
    r = R.Ring("", 8, 2, 10, 10 + 13, 5, 0)
    _, kr, vr, ks, vs, sv = R.inputs(r)
    k2, v2 = R.ring_after_commit(kr, vr, ks, vs, sv, r.p0)
    touched = set()
    for t in range(5):
        slot = 2 + (r.p0 + t - 2) % 8  # src/infer.cpp:611-613: token at position p goes to 2 + (p - 2) % W
        touched.add(slot)
        assert np.array_equal(k2[slot], ks[t]) and np.array_equal(v2[slot], vs[t])
    assert np.array_equal(k2[:2], sv[4]) and np.array_equal(v2[:2], vr[:2])
    rest = [s for s in range(2, 10) if s not in touched]
    assert np.array_equal(k2[rest], kr[rest]) and np.array_equal(v2[rest], vr[rest])
