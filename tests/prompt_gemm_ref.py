"""Float64 reference, input generators and case tables of the prompt-pass GEMM routes
(xh_op_prompt_matmul / xh_op_prompt_weight_image / xh_op_prompt_stage: gemm16.h behind its image
kernels, prefill_gemm16_kernel, prefill_gemm_kernel, the split producers and prefill_epi_kernel).

Definition: y[t][r] = sum_k x[t][k] W[r][k] with W the decoded weights (xh_dequantize_blocks for the
block formats, the oracle's per-code decode for the one-byte ones: the CPU suite pins both to the
converter).  Everything here is numpy; nothing needs a device.

Random parity bar (test_prompt_gemm's, for f32 accumulation of exact or 2^-22-split products):
  |y - ref| <= 1e-5 * sum_k |x W| + 1e-7.

Exact cases (asserted bitwise on the device, and shown exact here by exact_terms_ok):
  probes       x[t] is one-hot (1.0 at k_t): the split routes scale 1.0 to 2^14 (hi, lo = 0), every
               product is w or 0, so y[t][r] = W[r][k_t] whatever the order (+0 for -0: the sum starts
               at +0).
  sparse sums  x[t] has eight non-zeros m_k u_t with u_t a power of two and m_k odd integers: one in
               [2^21, 2^22), which fixes the row's scale, and seven in [2^12, 2^19).  Each has more than
               11 significant bits, so each needs its lo half (lo != 0), and hi + lo = m exactly (lo is a
               multiple of 2^-7 scaled, a normal f16).  Weights are integers in -2 .. 2.  Then
               sum_k |w_k| |m_k| <= 2 (2^22 + 7 2^19) < 2^24: every product (of x, of hi or of lo) and every
               partial sum in any order is an integer below 2^24 in units of u_t, hence exact in f32.
               Eight values of 22 bits each would reach 2^26 and round; that is why seven are shorter.
               XH_Q8 (0.01f * int8) has no integer weights: it takes the probes and the random bar only.
"""
import functools

import numpy as np

from oracle import oracle as O
from xalm_amd import _lib as L

ONE_BYTE = (L.F8_E4M3, L.F8_E5M2, L.Q8)
BLOCKS = (L.Q8_0, L.Q4_0, L.Q4_1, L.Q5_0, L.Q5_1, L.MXFP4)
F32_ROUTE_DTYPES = (L.F32, L.BF16, L.F16) + ONE_BYTE + BLOCKS
FRAG_DTYPES = (L.F16, L.F8_E4M3, L.F8_E5M2)
ROWMAJOR_DTYPES = (L.F16, L.F8_E4M3, L.F8_E5M2, L.Q8_0, L.Q4_0, L.Q5_0, L.MXFP4)
IMAGE_DTYPES = (L.F8_E4M3, L.F8_E5M2, L.MXFP4, L.Q8_0, L.Q4_0, L.Q5_0)
MX_E_LO, MX_E_HI = 114, 140  # MXFP4 scale bytes with an exact f16 image (include/xalm_hip.h)
# file layout of a 32-element block (include/xalm_synth.h): byte offsets of d, m, qh, e and the codes
BLOCK_FIELDS = {L.Q8_0: dict(d=0, q=2), L.Q4_0: dict(d=0, q=2), L.Q4_1: dict(d=0, m=2, q=4),
                L.Q5_0: dict(d=0, qh=2, q=6), L.Q5_1: dict(d=0, m=2, qh=4, q=8), L.MXFP4: dict(e=0, q=1)}
N_CODES = {L.Q8_0: 256, L.Q4_0: 16, L.Q4_1: 16, L.Q5_0: 32, L.Q5_1: 32, L.MXFP4: 16}


def elems(dtype):
    """Weights per 16-byte chunk of the f32-input kernel's decoder (WDec<DT>::E, pf_elems)."""
    if dtype == L.F32:
        return 4
    if dtype in (L.F16, L.BF16):
        return 8
    return 16 if dtype in ONE_BYTE + (L.Q8_0,) else 32


# ---- the split -----------------------------------------------------------------------------------
def split16(x):
    """prefill_split_kernel's exact f16 hi + lo of rows scaled into [2^14, 2^15) (float64 ref)"""
    m = np.abs(x).max(axis=1, keepdims=True)
    s = np.exp2(15 - np.ceil(np.log2(np.where(m > 0, m, 1.0)) + 1e-12))
    u = (x * s).astype(np.float32)
    hi = u.astype(np.float16)
    lo = (u - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def split_scale(x):
    """s_t of split_scale (prefill.h): row max = f 2^e, f in [0.5, 1) -> 2^(15 - e); 1 for a zero row."""
    m = np.abs(np.asarray(x, dtype=np.float64)).max(axis=1, keepdims=True)
    e = np.frexp(np.where(m > 0, m, 1.0))[1]
    return np.where(m > 0, np.exp2(15.0 - e), 1.0)


def split_exact(x):
    """The kernels' split of f32 rows in f32 arithmetic: (hi bits, lo bits, inv_s f32 [n])."""
    x = np.asarray(x, dtype=np.float32)
    s = split_scale(x).astype(np.float32)
    u = x * s
    hi = u.astype(np.float16)
    lo = (u - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16), (np.float32(1) / s)[:, 0]


def halves_value(hi, lo, inv_s):
    """(hi + lo) * inv_s in float64."""
    h = np.asarray(hi, np.uint16).view(np.float16).astype(np.float64)
    l = np.asarray(lo, np.uint16).view(np.float16).astype(np.float64)
    return (h + l) * np.asarray(inv_s, np.float64)[:, None]


# ---- float64 stages ------------------------------------------------------------------------------
def norm_weight_values(w, dtype):
    w = np.ascontiguousarray(w)
    return w.astype(np.float64) if dtype == L.F32 else (w.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def rmsnorm64(x, w, dtype, eps):
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * norm_weight_values(w, dtype)


def glu64(g, u, act):
    """act(g) * u as the oracle (src/infer.cpp:299-301): silu x / (1 + e^-x), or the tanh gelu."""
    g, u = np.asarray(g, np.float64), np.asarray(u, np.float64)
    if act == L.ACT_SILU:
        return g / (1.0 + np.exp(-g)) * u
    return 0.5 * g * (1.0 + np.tanh(0.797885 * (g + 0.044715 * g ** 3))) * u


def sum_slices64(part, part_s=None):
    v = np.asarray(part, np.float64).sum(axis=0)
    return v if part_s is None else v * np.asarray(part_s, np.float64)[:, None]


# ---- weights -------------------------------------------------------------------------------------
def f8_special(codes, dtype):
    return (codes & 0x7C) == 0x7C if dtype == L.F8_E5M2 else (codes & 0x7F) == 0x7F


@functools.lru_cache(maxsize=None)
def code_table(dtype):
    """The oracle's decode of the 256 codes of a one-byte dtype (float64)."""
    codes = np.arange(256, dtype=np.uint8)
    arr = codes.view(np.int8) if dtype == L.Q8 else codes
    return np.array([O.decode(dtype, arr, i) for i in range(256)], dtype=np.float64)


def decode_weights(dtype, w, rows, K):
    """File-layout weights -> float64 [rows][K]."""
    flat = np.ascontiguousarray(w).reshape(-1).view(np.uint8)
    if dtype == L.F32:
        v = flat.view(np.float32).astype(np.float64)
    elif dtype == L.F16:
        v = flat.view(np.float16).astype(np.float64)
    elif dtype == L.BF16:
        v = (flat.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    elif dtype in ONE_BYTE:
        v = code_table(dtype)[flat]
    else:
        v = L.dequantize_blocks(dtype, flat.reshape(rows, -1)).astype(np.float64)
    return v.reshape(rows, K)


def from_values(dtype, v):
    """Exactly representable values [rows][K] -> weights of an elementwise dtype (bytes [rows][row bytes])."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if dtype == L.F32:
        out = v
    elif dtype == L.F16:
        out = v.astype(np.float16)
    elif dtype == L.BF16:
        out = (v.view(np.uint32) >> 16).astype(np.uint16)
    else:
        tab = code_table(dtype)
        ok = np.where(~f8_special(np.arange(256), dtype) if dtype != L.Q8 else np.ones(256, bool))[0]
        lut = {float(tab[c]): c for c in ok[::-1]}  # +0 wins over -0
        out = np.array([lut[float(a)] for a in v.reshape(-1)], dtype=np.uint8).reshape(v.shape)
    return out.view(np.uint8).reshape(v.shape[0], -1)


def pack_blocks(dtype, q, d=None, m=None, e=None):
    """Codes q [rows][K] (0 .. N_CODES - 1; Q8_0: int8 as 0 .. 255) and per-block d, m (f16 values) or e
    (bytes), each [rows][K / 32] -> blocks in the file layout, uint8 [rows][K / 32 * block bytes]."""
    q = np.asarray(q).astype(np.int64)
    rows, K = q.shape
    nb, f, bb = K // 32, BLOCK_FIELDS[dtype], L.GQ_BLOCK_BYTES[dtype]
    out = np.zeros((rows, nb, bb), dtype=np.uint8)
    qb = q.reshape(rows, nb, 32)
    if dtype == L.Q8_0:
        out[:, :, f["q"]:] = qb.astype(np.uint8)
    else:
        out[:, :, f["q"]:f["q"] + 16] = ((qb[:, :, :16] & 15) | ((qb[:, :, 16:] & 15) << 4)).astype(np.uint8)
    if "qh" in f:
        bits = ((qb >> 4) & 1).astype(np.uint32)
        word = (bits << np.arange(32, dtype=np.uint32)).sum(axis=2).astype(np.uint32)
        out[:, :, f["qh"]:f["qh"] + 4] = word[..., None].view(np.uint8).reshape(rows, nb, 4)
    for name, val in (("d", d), ("m", m)):
        if name in f:
            h = np.broadcast_to(np.asarray(val, dtype=np.float16), (rows, nb)).copy()
            out[:, :, f[name]:f[name] + 2] = h[..., None].view(np.uint8).reshape(rows, nb, 2)
    if "e" in f:
        out[:, :, f["e"]] = np.broadcast_to(np.asarray(e, dtype=np.uint8), (rows, nb))
    return out.reshape(rows, nb * bb)


@functools.lru_cache(maxsize=None)
def mx_code_values():
    """The 16 e2m1 values at e = 127, by the dequantizer."""
    q = np.tile(np.arange(16), 2)[None, :]
    return L.dequantize_blocks(L.MXFP4, pack_blocks(L.MXFP4, q, e=127))[0, :16].astype(np.float64)


def small_int_weights(dtype, v):
    """Integer values in -2 .. 2, [rows][K], as weights of dtype (exactly: decode_weights gives v back)."""
    v = np.asarray(v, dtype=np.int64)
    if dtype not in BLOCKS:
        return from_values(dtype, v)
    if dtype == L.Q8_0:
        return pack_blocks(dtype, v & 255, d=1.0)
    if dtype == L.Q4_0:
        return pack_blocks(dtype, v + 8, d=1.0)
    if dtype == L.Q5_0:
        return pack_blocks(dtype, v + 16, d=1.0)
    if dtype in (L.Q4_1, L.Q5_1):
        return pack_blocks(dtype, v + 2, d=1.0, m=-2.0)
    lut = {float(val): c for c, val in reversed(list(enumerate(mx_code_values())))}
    return pack_blocks(dtype, np.vectorize(lambda a: lut[float(a)])(v), e=127)


def random_weights(rng, dtype, rows, K, wide=False):
    """Random codes: finite ones for fp8, no e = 255 and (unless wide) every e in 114 .. 140 for MXFP4."""
    if dtype in (L.F32, L.F16, L.BF16):
        v = (rng.standard_normal((rows, K)) * 0.05).astype(np.float32)
        v = v.astype(np.float16).astype(np.float32) if dtype == L.F16 else v
        v = (v.view(np.uint32) & 0xFFFF0000).view(np.float32) if dtype == L.BF16 else v
        return from_values(dtype, v)
    if dtype in ONE_BYTE:
        w = rng.integers(0, 256, size=(rows, K), dtype=np.uint8)
        if dtype != L.Q8:
            w[f8_special(w, dtype)] = 0x01
        return w
    nb = K // 32
    q = rng.integers(0, N_CODES[dtype], size=(rows, K))
    d = (0.01 * (1 + np.abs(rng.standard_normal((rows, nb)))) * rng.choice([-1.0, 1.0], size=(rows, nb)))
    m = rng.standard_normal((rows, nb)) * 0.05
    e = rng.integers(118, 137, size=(rows, nb))
    if wide:
        e[rows // 2, nb // 2] = 100
    return pack_blocks(dtype, q, d=d, m=m, e=e)


def coded_weights(dtype, rows, K, rowmajor):
    """The probes' weights: code (r + 37 k) mod the code count at [r][k], so every code (every nibble with
    every fifth bit; every finite one-byte code) stands at every block position within any N_CODES
    (one-byte: 256) consecutive rows; the blocks' d, m and e cycle through their extremes.  Row-major
    images hold d q in f16, so there |d q| stays below 65504 and e inside 114 .. 140."""
    r, k = np.arange(rows)[:, None], np.arange(K)[None, :]
    if dtype in (L.F32, L.F16, L.BF16):
        return random_weights(np.random.default_rng(7), dtype, rows, K)
    if dtype in ONE_BYTE:
        w = ((r + 37 * k) % 256).astype(np.uint8)
        if dtype != L.Q8:
            w[f8_special(w, dtype)] = 0x01
        return w
    nb = K // 32
    b = (np.arange(rows)[:, None] * 3 + np.arange(nb)[None, :])
    dl = np.array([1.0, -0.5, 2.0 ** -24, 256.0, -2.0 ** -14] if rowmajor else [1.0, -0.5, 2.0 ** -24, 65504.0, -65504.0])
    ml = np.array([0.0, -2.0, 65504.0, -2.0 ** -24, 0.3])
    el = np.array([MX_E_LO, MX_E_HI, 127, 120] if rowmajor else [127, 2, 250, MX_E_LO, MX_E_HI, 100])
    return pack_blocks(dtype, (r + 37 * k) % N_CODES[dtype], d=dl[b % len(dl)], m=ml[(b // 2) % len(ml)], e=el[b % len(el)])


# ---- inputs --------------------------------------------------------------------------------------
def random_x(rng, n, K):
    """Standard normal rows, scaled by 2^-20 .. 2^20 across the rows."""
    ex = np.linspace(-20, 20, n).round() if n > 1 else np.array([3.0])
    return (rng.standard_normal((n, K)) * np.exp2(ex)[:, None]).astype(np.float32)


def probe_ks(K, chunk, ks):
    """The k of the one-hot probes of a GEMM with K columns in ks slices and `chunk`-element 16-byte
    chunks: the first and last k of every slice, one k in every chunk (so both halves of every lane
    pair), stepping through the block positions, and every position 0 .. 31 of the first and last block."""
    sl = K // ks
    out = set()
    for s in range(ks):
        out |= {s * sl, (s + 1) * sl - 1}
    for c in range(K // chunk):
        out.add(c * chunk + (5 * c + 3) % chunk)
    out |= set(range(min(32, K))) | set(range(max(0, K - 32), K))
    return sorted(out)


def probe_x(ks_list, K):
    x = np.zeros((len(ks_list), K), dtype=np.float32)
    x[np.arange(len(ks_list)), ks_list] = 1.0
    return x


def sparse_case(rng, dtype, rows, K, n):
    """The exact sparse sums (module docstring): (x f32 [n][K], weights, integer W [rows][K], units [n])."""
    v = rng.integers(-2, 3, size=(rows, K))
    x = np.zeros((n, K), dtype=np.float64)
    units = np.exp2(np.linspace(-20, 20, n).round() if n > 1 else np.array([-3.0]))
    for t in range(n):
        cols = rng.choice(K, size=8, replace=False)
        mags = np.concatenate([rng.integers(2 ** 21, 2 ** 22, size=1), rng.integers(2 ** 12, 2 ** 19, size=7)]) | 1
        x[t, cols] = mags * rng.choice([-1, 1], size=8) * units[t]
    return x.astype(np.float32), small_int_weights(dtype, v), v, units


def exact_terms_ok(x, v, units):
    """Every product and every partial sum, in any order, an integer below 2^24 in the row's unit; also
    for the hi and lo halves of the split routes, with lo != 0 for every non-zero."""
    xi = np.asarray(x, np.float64) / units[:, None]
    if not np.array_equal(xi, np.round(xi)):
        return False
    if not np.all((np.abs(xi) @ np.abs(v).T.astype(np.float64)) < 2 ** 24):
        return False
    hi, lo, inv_s = split_exact(x)
    s = 1.0 / inv_s.astype(np.float64)
    h = hi.view(np.float16).astype(np.float64) / s[:, None]
    l = lo.view(np.float16).astype(np.float64) / s[:, None]
    if not np.array_equal(h + l, np.asarray(x, np.float64)):
        return False
    hu, lu = h / units[:, None], l / units[:, None]
    return bool(np.array_equal(hu, np.round(hu)) and np.array_equal(lu, np.round(lu)) and np.all((l != 0) == (xi != 0))
                and np.all((np.abs(hu) + np.abs(lu)) @ np.abs(v).T.astype(np.float64) < 2 ** 24))


# ---- K slicings ----------------------------------------------------------------------------------
WAVE_TARGET, PART_ROWS = 1024, 32 * 4 * 1024  # PF_WAVE_TARGET, PF_PART_ROWS (prefill.hip)


def forced_ks_ok(route, dtype, rows, K, ks, tile):
    """xh_op_prompt_matmul's rule for a forced slice count (include/xalm_hip.h), from the pickers."""
    if ks < 1 or ks & (ks - 1):
        return False
    if route == 0:
        return ks <= 8 and K % (ks * 64) == 0
    E = route if route > 0 else elems(dtype)
    unit = 8 * E if route > 0 or K % (8 * E) == 0 else 2 * E
    n_rt = -(-rows // tile)
    return ks <= 64 and K % (ks * unit) == 0 and (ks == 1 or ks * n_rt <= WAVE_TARGET) and ks * rows <= PART_ROWS


def gemm_cases(route_kind, dtype):
    """(K, ks) of the issue's shape list for a route: 6E (off the pipeline, one slice), 8E (one ring turn),
    16E in two slices; row-major: 64, 192, and 512 in four."""
    if route_kind == "rowmajor":
        return [(64, 0), (192, 0), (512, 4)]
    E = elems(dtype)
    base = [(8 * E, 0), (16 * E, 2)]
    return base if route_kind == "frag" else [(6 * E, 0)] + base


def row_cases(tile):
    """rows: under one 32-row tile, one launch tile and a ragged one, three and 33 rows."""
    return [8, tile + 8, 3 * tile + 33]
