"""Float64 reference of the single-token attention, its bar, and the planted-slot probes.

    s_t = (q_h . K[t, g]) / sqrt(head_dim),  p = softmax(s),  o_h = sum_t p_t V[t, g]

over the first kv_len ring slots, K and V decoded exactly from their f16 bits or e4m3 codes
(tests/kv8_ref.py's code table) and every operation in float64.

Bar, per output element i of head h.  Derived from the project's constants, not tuned:
    p . V is a matvec with weights p      2e-6 A_i,  A_i = sum_t p_t |v_t,i|      (tests/test_ops_gpu.py)
    the f32 scores carry an error of      ds = 2e-6 max_t sum_j |q_j k_t,j| / sqrt(head_dim) + 1e-7
    (a matvec row each), which enters every p_t through exp: p_t moves by at most a factor
    e^{+-2 ds} (its own score and the normaliser's), so o_i moves by at most 2 ds A_i
    bar_i = 2e-6 A_i + 2 ds A_i + 1e-7

Oracle headroom.  tests/test_attn_regimes_cpu.py requires the CPU oracle's f32 attention (O.mha; on
the e4m3 ring O.mha over the codes' exact f16 images) under this bar with at least 4x headroom on
every case of tests/attn_cases.py (the GPU sums in another order).  Worst err / bar of the oracle
over the table, measured on the CPU:
    f16 ring  0.024   e4m3 ring  0.026   (headroom 38x and more)
No case fell short, so the bar is not widened, and nothing is calibrated from GPU output.
That headroom holds for the table's seeded random cases only.  On the planted probes, the heads of the
group that are not planted see one large score over thousands of small ones; the oracle adds the
weights and the weighted rows one by one in f32, where a term below half an ulp of the running
sum is lost (sequential summation: up to n 2^-24 sum|terms|), and its err / bar there reaches 1.47
(128 x 4, e4m3 ring, kv_len 32768).  The CPU test prints that ratio and does not bound it; the device,
which sums a few terms per lane and then trees, is held to the bar on those heads too.

Planted-slot probes.  K[t] of every KV head is set to c q_h / |q_h| for one q head h of its group,
with c the smallest multiple of 16 for which the score of slot t exceeds every other slot's by more
than MARGIN = 110 (checked in float64 on the rounded row).  e^-110 < 2^-150 rounds to zero in f32,
so in any correct f32 evaluation every other weight is exactly 0, l is exactly 1, every other
split's merge weight is exactly 0, and the planted head's output is the decoded V[t] itself (as
values: a -0 of V comes out as the +0 of 0 + 1 * -0).
"""
import functools
import zlib

import numpy as np

from xalm_amd import _lib as L

MARGIN = 110.0


def decode_ring(ring, kv_dtype):
    """float64 values of ring rows: f16 bits (uint16) or e4m3 codes (uint8)."""
    if kv_dtype == L.F8_E4M3:
        import kv8_ref  # here: kv8_ref imports stage_ref, which imports this module
        return kv8_ref.image64(ring)
    return np.asarray(ring, np.uint16).view(np.float16).astype(np.float64)


@functools.lru_cache(maxsize=2)
def inputs(row):
    """(kb, vb, q) of a row of tests/attn_cases.py, seeded by the row: a whole ring of standard
    normal K and V elements and q of 0.5 standard deviations (test_mha's regime).  Shared by every
    case of the row: copy before planting."""
    rng = np.random.default_rng(zlib.crc32(repr(tuple(row)).encode()))
    kv_dim, n_heads = row.n_kv * row.head_dim, row.n_kv * row.qpk
    kb = quantize_row(rng.standard_normal((row.msl, kv_dim)), row.kv_dtype)
    vb = quantize_row(rng.standard_normal((row.msl, kv_dim)), row.kv_dtype)
    q = (rng.standard_normal(n_heads * row.head_dim) * 0.5).astype(np.float32)
    for a in (kb, vb, q):
        a.setflags(write=False)
    return kb, vb, q


def attention64(k64, v64, q, head_dim, kv_len, n_heads, n_kv, heads=None):
    """(att, bar, off) float64 [n_heads * head_dim] x 2 and [n_heads]: the attention output, its
    bar, and per head the largest softmax weight off the head's largest one (the probes'
    precondition).  heads: only these (the rest stay NaN)."""
    qpk = n_heads // n_kv
    q = np.asarray(q, np.float64)
    att, bar, off = (np.full(n, np.nan) for n in (n_heads * head_dim, n_heads * head_dim, n_heads))
    scale = 1.0 / np.sqrt(np.float64(head_dim))
    for h in range(n_heads) if heads is None else heads:
        hs = slice(h * head_dim, (h + 1) * head_dim)
        ks = slice(h // qpk * head_dim, (h // qpk + 1) * head_dim)
        k, v = k64[:kv_len, ks], v64[:kv_len, ks]
        s = (k @ q[hs]) * scale
        e = np.exp(s - s.max())
        p = e / e.sum()
        att[hs] = p @ v
        a = p @ np.abs(v)
        ds = 2e-6 * float((np.abs(k) @ np.abs(q[hs])).max()) * scale + 1e-7
        bar[hs] = 2e-6 * a + 2.0 * ds * a + 1e-7
        top = int(np.argmax(s))
        e[top] = 0.0
        off[h] = e.max() if kv_len > 1 else 0.0
    return att, bar, off


def quantize_row(row, kv_dtype):
    """A float row as ring elements: f16 bits, or e4m3 codes by the host definition."""
    row = np.ascontiguousarray(row, np.float32)
    return L.f8_e4m3_from_f32(row) if kv_dtype == L.F8_E4M3 else row.astype(np.float16).view(np.uint16)


def plant(kb, q, t, head, kv_dtype, head_dim, kv_len, n_heads, n_kv):
    """Set K[t] of every KV head to c * q_h / |q_h| in place (h = the q head `head` of its group)
    and return c.  Raises if no c within the ring type's range gives the margin."""
    qpk = n_heads // n_kv
    scale = 1.0 / np.sqrt(np.float64(head_dim))
    lim = 448.0 if kv_dtype == L.F8_E4M3 else 60000.0
    worst_c = 0
    for g in range(n_kv):
        h = g * qpk + head
        qh = np.asarray(q[h * head_dim:(h + 1) * head_dim], np.float64)
        cols = slice(g * head_dim, (g + 1) * head_dim)
        s = decode_ring(kb[:kv_len, cols], kv_dtype) @ qh * scale
        s[t] = -np.inf
        other = float(s.max()) if kv_len > 1 else 0.0
        u = qh / np.linalg.norm(qh)
        c = 16 * int(np.ceil((MARGIN + 1.0 + max(other, 0.0)) / (np.linalg.norm(qh) * scale) / 16))
        while True:
            if c * np.abs(u).max() > lim:
                raise ValueError(f"no planted row within +-{lim} reaches the margin")
            row = quantize_row(c * u, kv_dtype)
            if float(decode_ring(row, kv_dtype) @ qh) * scale - other > MARGIN + 0.5:
                break
            c += 16
        kb[t, cols] = row
        worst_c = max(worst_c, c)
    return worst_c


def values_equal(got, want):
    """got == want as float values (a -0 and a +0 are equal; NaN never is)."""
    return bool(np.all(np.asarray(got, np.float32) == np.asarray(want, np.float32)))
