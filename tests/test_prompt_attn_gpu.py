"""The prompt-pass attention kernels (prefill.h) op by op against the float64 reference of
tests/prompt_attn_ref.py: xh_op_prompt_attn (prefill_fa_kernel, prefill_fa2_kernel and its history
splits, prefill_fa_merge_kernel<false>) and xh_op_prompt_attn_ring (prefill_fa2_ring_kernel,
prefill_fa_merge_kernel<true>, prefill_ring_commit_kernel), through the launch code of the passes.

Every row, head and element of `out` is held to the derived bar of the reference module (conditions
checked on the CPU by tests/test_prompt_attn_cpu.py); each case prints its worst err / bar (-s).
"""

import numpy as np
import pytest

from xalm_amd import _lib as L

import prompt_attn_ref as R

pytestmark = pytest.mark.gpu

E_INVALID = 1


def run_causal(c):
    q, k, v = R.inputs(c)
    return L.op_prompt_attn(q, k, v, c.pos0, c.hd, c.n_heads, c.n_kv, c.mode, c.nsplit)


def check(got, c):
    assert np.all(np.isfinite(got))
    r = R.ratio(got, c)
    print(f"\n{R.case_id(c)}: worst err / bar = {r:.4f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("c", R.CAUSAL_CASES, ids=R.case_id)
def test_causal(c):
    """Head shapes in both modes (ragged query tiles, a wave with no rows, rows that see 1 .. 64
    keys), tile and stage edges of the shared-tile kernel, forced and chosen history splits over
    2400 and 700 slots, and the peaked softmax whose max moves at the end of the walk."""
    check(run_causal(c), c)


@pytest.mark.parametrize("c", R.RING_CASES, ids=R.case_id)
def test_ring(c):
    """Ring passes: small windows with the wrap from slot L - 1 to slot 2 inside them, and a long
    window in forced and chosen splits, some of them invisible to a workgroup's later rows.  The
    ring comes back exactly as the commit leaves it."""
    q, kr, vr, ks, vs, sv = R.inputs(c)
    got, k2, v2 = L.op_prompt_attn_ring(q, kr, vr, ks, vs, sv, c.p0, c.n_heads, c.n_kv, c.nsplit)
    check(got, c)
    want_k, want_v = R.ring_after_commit(kr, vr, ks, vs, sv, c.p0)
    assert np.array_equal(k2, want_k) and np.array_equal(v2, want_v)


def bits(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("nsplit", [3, 0])
def test_split_case_repeats_bit_identically(nsplit):
    c = R.Causal("splits", 8, 2, 128, 40, 2400, 1, nsplit, "rand")
    assert np.array_equal(bits(run_causal(c)), bits(run_causal(c)))


@pytest.mark.parametrize("shape", R.SPLIT_SHAPES + [(16, 2, 128), (8, 4, 128)], ids=str)
@pytest.mark.parametrize("n,pos0", [(70, 45), (40, 2400)])
def test_shared_tiles_one_split_bit_identical_to_per_wave(shape, n, pos0):
    """prefill_fa2_kernel repeats prefill_fa_kernel's per-wave arithmetic in the same order."""
    a = run_causal(R.Causal("", *shape, n, pos0, 1, 1, "rand"))
    b = run_causal(R.Causal("", *shape, n, pos0, 2, 0, "rand"))
    assert np.array_equal(bits(a), bits(b))


SENTINEL = 0x7FC0BEEF


def last_error():
    msg = L.lib().xh_last_error(None)
    return msg.decode() if msg else ""


def causal_rc(n_heads, n_kv, hd, n, pos0, mode, nsplit):
    q = np.zeros((n, n_heads * hd), np.float32)
    kv = np.zeros((pos0 + n, n_kv * hd), np.uint16)
    out = np.full(q.shape, SENTINEL, np.uint32)
    rc = L.lib().xh_op_prompt_attn(L.ptr(out), L.ptr(q), L.ptr(kv), L.ptr(kv), n, pos0, hd, n_heads, n_kv, mode, nsplit)
    return rc, out


@pytest.mark.parametrize("args", [
    (6, 4, 128, 8, 0, 1, 0),      # 6 q heads over 4 KV heads
    (8, 2, 32, 8, 0, 1, 0),       # head_dim 32
    (8, 2, 128, 8, 2400, 1, 10),  # 2400 / 64 / 4 = 9 splits at the most
    (8, 2, 128, 8, 200, 1, 2),    # under 4 stages of history: one split
    (8, 2, 128, 8, 2400, 2, 2),   # splits under the per-wave kernel
    (8, 2, 64, 8, 2400, 1, 2),    # ... and at head_dim 64
    (8, 2, 128, 8, 0, 0, 0),      # mode 0 is not this hook's
    (8, 2, 128, 8, 0, 1, -1),
], ids=str)
def test_prompt_attn_rejects(args):
    rc, out = causal_rc(*args)
    assert rc == E_INVALID and last_error()
    assert np.all(out == SENTINEL)  # nothing ran


@pytest.mark.parametrize("L_,p0,m,heads,nsplit", [
    (66, 66, 2, (8, 2), 1),      # m < 3
    (66, 66, 65, (8, 2), 1),     # m > W
    (66, 65, 8, (8, 2), 1),      # p0 < L
    (3, 66, 3, (8, 2), 1),       # W < 2
    (66, 66, 8, (6, 4), 1),
    (66, 66, 8, (8, 2), 2),      # W / 64 / 4 = 0: one split
    (2306, 3306, 8, (8, 2), 10),
], ids=str)
def test_prompt_attn_ring_rejects(L_, p0, m, heads, nsplit):
    n_heads, n_kv = heads
    kv = n_kv * 128
    q = np.zeros((max(m, 1), n_heads * 128), np.float32)
    ring = np.full((max(L_, 1), kv), 0x3C00, np.uint16)
    ring2 = ring.copy()
    st = np.zeros((max(m, 1), kv), np.uint16)
    sv = np.zeros((max(m, 1), 2, kv), np.uint16)
    out = np.full(q.shape, SENTINEL, np.uint32)
    rc = L.lib().xh_op_prompt_attn_ring(L.ptr(out), L.ptr(ring), L.ptr(ring2), L.ptr(q), L.ptr(st), L.ptr(st), L.ptr(sv), m,
                                        p0, L_, n_heads, n_kv, nsplit)
    assert rc == E_INVALID and last_error()
    assert np.all(out == SENTINEL) and np.all(ring == 0x3C00) and np.all(ring2 == 0x3C00)


def test_null_pointers_are_rejected():
    q = np.zeros((4, 1024), np.float32)
    assert L.lib().xh_op_prompt_attn(None, L.ptr(q), L.ptr(q), L.ptr(q), 4, 0, 128, 8, 2, 1, 0) == E_INVALID
    assert last_error()
    assert L.lib().xh_op_prompt_attn_ring(L.ptr(q), None, None, L.ptr(q), None, None, None, 4, 66, 66, 8, 2, 1) == E_INVALID
    assert last_error()
