"""The stage sweep's CPU half: the case table covers every launch shape the dispatch can reach, and
the bars of tests/stage_ref.py hold, with headroom, for a correct f32 evaluation (no GPU).
"""
import ctypes
import json

import pytest

from conftest import fixture_path
from xalm_amd import _lib as L
from xalm_amd.model import Model

import stage_cases as SC
import stage_ref as SR

NMAX, WO_MAX = 32768, 8192
ROLE_NAME = {L.ROLE_QKV: "QKV", L.ROLE_GLU: "GLU", L.ROLE_RESID: "RESID", L.ROLE_LOGITS: "LOGITS"}


def shape_name(s):
    return L.SHAPE_NAMES[s & ~L.SHAPE_BIG_LDS] + ("+lds" if s & L.SHAPE_BIG_LDS else "")


def reachable(role, nmax):
    """{(dtype, shape): (smallest n, largest n)} over every multiple of 32 up to nmax."""
    cells = {}
    for dt in SC.ALL:
        for n in range(32, nmax + 1, 32):
            s = L.gemv_shape(role, dt, n)
            assert s >= 0, (role, dt, n)
            lo, hi = cells.get((dt, s), (n, n))
            cells[(dt, s)] = (min(lo, n), max(hi, n))
    return cells


def test_case_table_covers_every_reachable_shape():
    """Every (role, dtype, shape) xh_gemv_shape can return is run by the table at the smallest and
    at the largest input length that select it (Wo: the largest n_heads * head_dim <= 8192)."""
    table = SC.CASES + SC.EDGES
    hit = {
        "dim": {(dt, c.dim) for c in table for dt in c.dtypes},
        "W2": {(dt, c.hidden) for c in table for dt in c.dtypes},
        "Wo": {(dt, c.heads * c.head_dim) for c in table for dt in c.dtypes},
    }
    missing, n_cells = [], 0
    for role, key, nmax in ((L.ROLE_QKV, "dim", NMAX), (L.ROLE_GLU, "dim", NMAX), (L.ROLE_LOGITS, "dim", NMAX),
                            (L.ROLE_RESID, "W2", NMAX), (L.ROLE_RESID, "Wo", WO_MAX)):
        for (dt, s), ends in sorted(reachable(role, nmax).items()):
            n_cells += 1
            for n in set(ends):
                if (dt, n) not in hit[key]:
                    missing.append(f"{ROLE_NAME[role]} ({key}) {SC.DT_NAME[dt]} {shape_name(s)}: no case at n = {n}")
    assert not missing, "\n".join(missing)
    assert n_cells >= 5 * 11 * 2  # every role and dtype takes at least two shapes
    # all ten shapes are reachable, and every one of them both with and without the raised LDS limit
    # where its range crosses 64 KiB
    seen = {s & ~L.SHAPE_BIG_LDS for role in ROLE_NAME for (dt, s) in reachable(role, NMAX)}
    assert seen == set(range(len(L.SHAPE_NAMES))), seen


def test_case_table_holds_the_balanced_grids_and_the_edges():
    """What the enumeration cannot ask for: the two balanced grids past 2048 output rows
    (gemv_blocks' round-up to whole multiples of 256), lengths inside a shape where the row loops
    end differently, and one case per epilogue / config edge, each with F16 and an fp8 dtype."""
    table = SC.CASES + SC.EDGES
    pairs = [(c, dt) for c in table for dt in c.dtypes]
    for dt in (L.F8_E4M3, L.F8_E5M2, L.Q8):
        assert any(d == dt and shape_name(L.gemv_shape(L.ROLE_QKV, d, c.dim)) == "PF2PB" and
                   (c.heads + 2 * c.kv_heads) * c.head_dim > 2048 for c, d in pairs), dt
    for dt in (L.Q8_0, L.Q4_0, L.Q4_1, L.Q5_0, L.Q5_1):
        assert any(d == dt and shape_name(L.gemv_shape(L.ROLE_GLU, d, c.dim)) == "GQ" and 2 * c.hidden > 2048
                   for c, d in pairs), dt
    assert any(c.dim == 3072 and d == L.F16 for c, d in pairs)       # a partial last step of PF2
    assert any(c.dim == 5120 for c in table)                         # the rmsnorm prologue past 4096
    assert any(c.hidden == 11008 and d == L.Q4_0 for c, d in pairs)  # the staged gguf W2
    edges = {
        "odd vocab": lambda c: c.vocab == 1031,
        "F32 norm weights": lambda c: c.norm_dt == L.F32,
        "GELU": lambda c: c.act == L.ACT_GELU,
        "qkv_clip": lambda c: c.clip == 0.5,
        "half rotary + wrapping prefill": lambda c: c.rotary == c.head_dim // 2 and c.prefill == 70 > SC.MSL,
        "tied embeddings": lambda c: c.tied == 1,
        "fused head shape": lambda c: c.head_dim == 128 and c.heads // c.kv_heads == 4,
        "unfused head shape": lambda c: c.head_dim == 64 and c.heads // c.kv_heads == 2,
    }
    for name, has in edges.items():
        dts = {d for c in table if has(c) for d in c.dtypes}
        assert L.F16 in dts and dts & {L.F8_E4M3, L.F8_E5M2}, name


def cell_map():
    return {f"{ROLE_NAME[role]} {SC.DT_NAME[dt]} {shape_name(s)}": list(ends)
            for role in ROLE_NAME for (dt, s), ends in sorted(reachable(role, NMAX).items())}


def test_dispatch_cells_are_the_recorded_ones():
    """The whole map (role, dtype, shape) -> [smallest n, largest n] equals the recorded one
    (tests/golden/gemv_shape_cells.json), so a threshold that moves fails here even where the moved
    boundary lands on a length the table already runs.  A deliberate dispatch change re-records the
    map (python tests/test_stages_cpu.py) and revisits the case table."""
    recorded = json.load(open(fixture_path("gemv_shape_cells.json")))
    now = cell_map()
    diff = {k: (recorded.get(k), now.get(k)) for k in sorted(set(recorded) | set(now)) if recorded.get(k) != now.get(k)}
    assert not diff, diff


def test_gemv_shape_rejects_what_has_no_matvec():
    assert L.gemv_shape(L.ROLE_QKV, L.U8, 4096) == -1       # no matvec for the dtype
    assert L.gemv_shape(7, L.F16, 4096) == -1                # no such role
    assert L.gemv_shape(L.ROLE_QKV, L.F16, 4100) == -1       # not whole 32-element blocks
    assert L.gemv_shape(L.ROLE_RESID, L.F16, 40992) == -1    # the input does not fit the LDS
    assert L.gemv_shape(L.ROLE_RESID, L.F32, 40704) == (9 | L.SHAPE_BIG_LDS)  # the last length that fits
    # the shapes the flagship configurations are tuned on: f16 / fp8 Mistral-7B
    assert shape_name(L.gemv_shape(L.ROLE_QKV, L.F16, 4096)) == "Q384"
    assert shape_name(L.gemv_shape(L.ROLE_QKV, L.F8_E4M3, 4096)) == "PF2PB"
    assert shape_name(L.gemv_shape(L.ROLE_GLU, L.F16, 4096)) == "PF2P"
    assert shape_name(L.gemv_shape(L.ROLE_RESID, L.F8_E4M3, 14336)) == "W2K"
    assert shape_name(L.gemv_shape(L.ROLE_RESID, L.F16, 14336)) == "PF8"
    assert shape_name(L.gemv_shape(L.ROLE_GLU, L.Q4_0, 4096)) == "GQ"
    assert shape_name(L.gemv_shape(L.ROLE_RESID, L.Q4_0, 14336)) == "GQL"


def test_create_rejects_an_input_wider_than_the_lds():
    """hidden_dim 40992: the W2 input image (64 + 161 KiB as f32 chunks) exceeds the 160 KiB a
    workgroup can hold; xh_create says so, before it looks for a device.  No forward is run."""
    c = SC.config(SC.case(256, 40992))
    with pytest.raises(L.XhError, match="LDS"):
        Model(c)
    ctx = ctypes.c_void_p()
    assert L.lib().xh_create(ctypes.byref(c), 0, ctypes.byref(ctx)) == 1 and not ctx  # XH_E_INVALID


WORST = {}


@pytest.mark.parametrize("c,wdt", SC.all_cases(), ids=[SC.case_id(c, d) for c, d in SC.all_cases()])
def test_oracle_is_within_the_bars(c, wdt):
    """The stages composed from the oracle's f32 ops stay under every bar with 4x headroom."""
    W = SR.host_weights(c, wdt)
    ratio = SR.check_stages(c, wdt, W, SR.oracle_observe(c, wdt, W))
    for stage, r in ratio.items():
        if r > WORST.get(stage, (0.0, ""))[0]:
            WORST[stage] = (r, SC.case_id(c, wdt))
    print({k: round(v, 4) for k, v in ratio.items()})
    # k, v: rounding to f16 alone is up to half an ulp, half of the bar's one-ulp term, in every
    # correct evaluation and whatever the summation order; the 4x applies to the f32 part beside it
    # ((ulp / 2 + b32 / 4) / (ulp + b32) <= 1 / 2)
    for stage, r in ratio.items():
        assert r <= (0.5 if stage in ("k", "v") else 0.25), (stage, ratio)


def test_oracle_headroom_summary():
    """Prints the worst err / bar per stage over the cases run before it (python -m pytest -s)."""
    for stage in SR.STAGES:
        if stage in WORST:
            print(f"oracle worst err / bar  {stage:9s} {WORST[stage][0]:.4f}  {WORST[stage][1]}")


if __name__ == "__main__":  # re-record the dispatch map after a deliberate change
    with open(fixture_path("gemv_shape_cells.json"), "w") as f:
        json.dump(cell_map(), f, indent=0, sort_keys=True)
        f.write("\n")
