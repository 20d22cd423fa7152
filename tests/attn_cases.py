"""The cases of the decode-attention regime sweep (tests/attn_ref.py, test_attn_regimes_cpu.py,
test_attn_regimes_gpu.py).

A row is one (route, KV dtype, head shape, KV heads, max_seq_len); a case is a row at one kv_len.
The kv_len values are decided by the code's own plan, not by taste: test_attn_regimes_cpu.py sweeps
xh_attn_plan over every kv_len of 1..max_seq_len of every row and asserts that LENS holds the first
and the last kv_len of every regime the row can reach.  Deleting a value, or moving a constant in
attention.h / attn_wo.h / attn_nsplit, fails that test; it then prints what is missing.

A regime is what the plan reports, without the raw sizes:
    route and KV dtype (the row), then
    n_active class      1, 2, 3, 4, 5..64 (5), 65 and up (65)
    rounds class        of a whole split and of the last one: 1, 2, 3, an even count >= 4 (4), an odd one (5)
    ragged              kv_len % 4 != 0 (then kv_len % 16 and kv_len % step are non-zero too)
    merge form, (m, l) loads per lane, fused stage form

Rows.  Split route (xh_op_mha / xh_op_mha8), f16 and e4m3 rings, (head_dim, q heads per KV head):
(128,4) (128,8) (128,1) (64,1) (64,4) (32,2) (16,1) (16,2) (16,4) (256,8) with 1 or 2 KV heads, and
(16,2) with 8 (the only rows whose splits grow past 256 slots: with 1 or 2 KV heads the split count
follows max_seq_len up to 128).  max_seq_len is the smallest multiple of 256 that reaches the
row's last regime, 32768 at most: 128 active splits need 32768; (16,1) stops at 16640, the smallest
ring with 65 active splits under 15 merge groups.  Fused route (the one-layer model), f16 ring:
(128,4) (128,8) (64,4) (16,2), split floors 128, 128, 256 and 1024 slots, max_seq_len the smallest
that reaches "arrives merged" with every split active.

The largest ring is 32768 x 128 elements (8 MiB of f16).
"""
from collections import namedtuple

from xalm_amd import _lib as L

Row = namedtuple("Row", "fused kv_dtype head_dim qpk n_kv msl")

SPLIT_SHAPES = [  # (head_dim, qpk, n_kv, max_seq_len)
    (128, 4, 1, 32768), (128, 8, 1, 4096), (128, 1, 1, 32768), (64, 1, 1, 32768), (64, 4, 2, 4096), (32, 2, 1, 32768),
    (16, 1, 1, 16640), (16, 2, 1, 32768), (16, 4, 2, 4096), (256, 8, 1, 2048), (16, 2, 8, 32768),
]
FUSED_SHAPES = [(128, 4, 1, 2048), (128, 8, 1, 2048), (64, 4, 1, 4096), (16, 2, 1, 8192)]
ROWS = [Row(0, dt, *s) for dt in (L.F16, L.F8_E4M3) for s in SPLIT_SHAPES] + [Row(1, L.F16, *s) for s in FUSED_SHAPES]

# cases the enumeration does not ask for: the defect's instances named in the issue and the like
EXTRA = {
    Row(0, L.F16, 64, 1, 1, 32768): (20000,),
    Row(0, L.F8_E4M3, 64, 1, 1, 32768): (20000,),
}


def row_id(r):
    return f"{'fused' if r.fused else 'split'}-{'e4m3' if r.kv_dtype == L.F8_E4M3 else 'f16'}-{r.head_dim}x{r.qpk}kv{r.n_kv}-msl{r.msl}"


def plan(r, kv_len):
    return L.attn_plan(r.head_dim, r.qpk * r.n_kv, r.n_kv, r.msl, r.kv_dtype, r.fused, kv_len)


def n_active_class(n):
    return n if n <= 4 else 5 if n <= 64 else 65


def rounds_class(n):
    return n if n <= 3 else 4 if n % 2 == 0 else 5


def regime(p, kv_len):
    return (n_active_class(p.n_active), rounds_class(p.rounds_full), rounds_class(p.rounds_last), int(kv_len % 4 != 0),
            p.merge_mb, p.merge_nc, p.stage)


REGIME_FIELDS = "n_active class, rounds (whole split), rounds (last split), ragged, merge form, (m, l) loads, stage"


def reachable(r):
    """{regime: [first kv_len, last kv_len]} of the row over kv_len = 1..max_seq_len."""
    out = {}
    for kv_len in range(1, r.msl + 1):
        out.setdefault(regime(plan(r, kv_len), kv_len), [kv_len, kv_len])[1] = kv_len
    return out


def probe_slots(r, kv_len):
    """The planted slots of a case: the first and last slot of the first, second and last active
    split, the slot on each side of every round boundary of the first split, and kv_len - 1."""
    p = plan(r, kv_len)
    t = set()
    for s in sorted({0, min(1, p.n_active - 1), p.n_active - 1}):
        t |= {s * p.T, min(kv_len, (s + 1) * p.T) - 1}
    for b in range(p.step, min(p.T, kv_len), p.step):
        t |= {b - 1, b}
    t.add(kv_len - 1)
    return sorted(t)


def probe_lens(r):
    """The cases of a row that carry planted probes: per (n_active class, merge form, loads, stage)
    the last kv_len of LENS that has it."""
    pick = {}
    for kv_len in lens(r):
        p = plan(r, kv_len)
        pick[(n_active_class(p.n_active), p.merge_mb, p.merge_nc, p.stage)] = kv_len
    return sorted(set(pick.values()))


def lens(r):
    return tuple(sorted(set(LENS[row_id(r)]) | set(EXTRA.get(r, ()))))


# the first and the last kv_len of every regime of every row (test_attn_regimes_cpu.py checks it)
LENS = {
    "split-f16-128x4kv1-msl32768": (
        1, 4, 127, 128, 129, 132, 255, 256, 257, 260, 383, 384, 385, 388, 511, 512, 513, 516, 639, 640, 641,
        644, 767, 768, 769, 772, 895, 896, 897, 900, 1023, 1024, 1025, 1028, 1153, 1156, 1919, 1920, 2047, 2048,
        2049, 2052, 2177, 2180, 3967, 3968, 4095, 4096, 4097, 4100, 4225, 4228, 16255, 16256, 16383, 16384,
        16385, 16388, 16513, 16516, 32639, 32640, 32767, 32768,
    ),
    "split-f16-128x8kv1-msl4096": (
        1, 4, 127, 128, 129, 132, 255, 256, 257, 260, 383, 384, 385, 388, 511, 512, 513, 516, 639, 640, 641,
        644, 767, 768, 769, 772, 895, 896, 897, 900, 1023, 1024, 1025, 1028, 1153, 1156, 1919, 1920, 2047, 2048,
        2049, 2052, 2177, 2180, 3967, 3968, 4095, 4096,
    ),
    "split-f16-128x1kv1-msl32768": (
        1, 4, 127, 128, 129, 132, 255, 256, 257, 260, 383, 384, 385, 388, 511, 512, 513, 516, 639, 640, 641,
        644, 767, 768, 769, 772, 895, 896, 897, 900, 1023, 1024, 1025, 1028, 1153, 1156, 8063, 8064, 8191, 8192,
        8193, 8196, 8321, 8324, 16255, 16256, 16383, 16384, 16385, 16388, 16513, 16516, 32639, 32640, 32767,
        32768,
    ),
    "split-f16-64x1kv1-msl32768": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 15359, 15360,
        15361, 15364, 16383, 16384, 16385, 16388, 32767, 32768,
    ),
    "split-f16-64x4kv2-msl4096": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 4095, 4096,
    ),
    "split-f16-32x2kv1-msl32768": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 15359, 15360,
        15361, 15364, 16383, 16384, 16385, 16388, 32767, 32768,
    ),
    "split-f16-16x1kv1-msl16640": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 15359, 15360,
        15361, 15364, 16383, 16384, 16385, 16388, 16639, 16640,
    ),
    "split-f16-16x2kv1-msl32768": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 15359, 15360,
        15361, 15364, 16383, 16384, 16385, 16388, 32767, 32768,
    ),
    "split-f16-16x4kv2-msl4096": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 4095, 4096,
    ),
    "split-f16-256x8kv1-msl2048": (
        1, 4, 63, 64, 65, 68, 127, 128, 129, 132, 191, 192, 193, 196, 255, 256, 257, 260, 319, 320, 321, 324,
        383, 384, 385, 388, 447, 448, 449, 452, 511, 512, 513, 516, 575, 576, 577, 580, 639, 640, 641, 644, 703,
        704, 705, 708, 767, 768, 769, 772, 831, 832, 833, 836, 895, 896, 897, 900, 959, 960, 961, 964, 1023,
        1024, 1025, 1028, 1089, 1092, 1153, 1156, 1217, 1220, 1855, 1856, 1919, 1920, 1983, 1984, 2047, 2048,
    ),
    "split-f16-16x2kv8-msl32768": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 32767, 32768,
    ),
    "split-e4m3-128x4kv1-msl32768": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 2047, 2048,
        2049, 2052, 4095, 4096, 4097, 4100, 16383, 16384, 16385, 16388, 32767, 32768,
    ),
    "split-e4m3-128x8kv1-msl4096": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 2047, 2048,
        2049, 2052, 4095, 4096,
    ),
    "split-e4m3-128x1kv1-msl32768": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 8191, 8192,
        8193, 8196, 16383, 16384, 16385, 16388, 32767, 32768,
    ),
    "split-e4m3-64x1kv1-msl32768": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 15359, 15360,
        15361, 15364, 16383, 16384, 16385, 16388, 32767, 32768,
    ),
    "split-e4m3-64x4kv2-msl4096": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 4095, 4096,
    ),
    "split-e4m3-32x2kv1-msl32768": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 15359, 15360,
        15361, 15364, 16383, 16384, 16385, 16388, 32767, 32768,
    ),
    "split-e4m3-16x1kv1-msl16640": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 15359, 15360,
        15361, 15364, 16383, 16384, 16385, 16388, 16639, 16640,
    ),
    "split-e4m3-16x2kv1-msl32768": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 15359, 15360,
        15361, 15364, 16383, 16384, 16385, 16388, 32767, 32768,
    ),
    "split-e4m3-16x4kv2-msl4096": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 4095, 4096,
    ),
    "split-e4m3-256x8kv1-msl2048": (
        1, 4, 127, 128, 129, 132, 255, 256, 257, 260, 383, 384, 385, 388, 511, 512, 513, 516, 639, 640, 641,
        644, 767, 768, 769, 772, 895, 896, 897, 900, 1023, 1024, 1025, 1028, 1153, 1156, 1919, 1920, 2047, 2048,
    ),
    "split-e4m3-16x2kv8-msl32768": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 32767, 32768,
    ),
    "fused-f16-128x4kv1-msl2048": (
        1, 4, 127, 128, 129, 132, 255, 256, 257, 260, 383, 384, 385, 388, 511, 512, 513, 516, 1023, 1024, 1025,
        1028, 1137, 1140, 1807, 1808, 2047, 2048,
    ),
    "fused-f16-128x8kv1-msl2048": (
        1, 4, 127, 128, 129, 132, 255, 256, 257, 260, 383, 384, 385, 388, 511, 512, 513, 516, 1023, 1024, 1025,
        1028, 1137, 1140, 1807, 1808, 2047, 2048,
    ),
    "fused-f16-64x4kv1-msl4096": (
        1, 4, 255, 256, 257, 260, 511, 512, 513, 516, 767, 768, 769, 772, 1023, 1024, 1025, 1028, 4095, 4096,
    ),
    "fused-f16-16x2kv1-msl8192": (
        1, 4, 1023, 1024, 1025, 1028, 2047, 2048, 2049, 2052, 3071, 3072, 3073, 3076, 4095, 4096, 4097, 4100,
        8191, 8192,
    ),
}
