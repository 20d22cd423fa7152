"""Numpy statement of XH_OPT_PREFILL_I8 (include/xalm_hip.h): the per-block int8 quantiser in f32 and the GEMM of
the defined operands in float64."""
import numpy as np

import prompt_gemm_ref as G
from xalm_amd import _lib as L

BIAS = {L.Q8_0: 0, L.Q4_0: 8, L.Q4_1: 0, L.Q5_0: 16, L.Q5_1: 0}
F32 = np.float32


def quantise(hi, lo):
    """f16 bits hi, lo [n][K] -> (codes int8 [n][K], scales f32 [n][K / 32][2] = {dx, sx}), every step in f32."""
    v = np.asarray(hi, np.uint16).view(np.float16).astype(F32) + np.asarray(lo, np.uint16).view(np.float16).astype(F32)
    vb = v.reshape(v.shape[0], -1, 32)
    amax = np.abs(vb).max(axis=2)
    with np.errstate(divide="ignore"):
        inv = np.where(amax > 0, F32(127) / amax, F32(0)).astype(F32)
    q = np.clip(np.rint(vb * inv[..., None]), -127, 127).astype(np.int8)
    dx = amax / F32(127)
    sx = dx * q.sum(axis=2, dtype=np.int32).astype(F32)
    return q.reshape(v.shape), np.stack([dx, sx], axis=2).astype(F32)


def block_parts(dtype, w, rows, K):
    """File-layout blocks -> d, m float64 [rows][K / 32] and the integer codes less the bias [rows][K / 32][32]."""
    f, blk = G.BLOCK_FIELDS[dtype], np.ascontiguousarray(w).reshape(rows, K // 32, L.GQ_BLOCK_BYTES[dtype])
    half = lambda o: blk[..., o:o + 2].copy().view(np.float16)[..., 0].astype(np.float64)
    d, m = half(f["d"]), half(f["m"]) if "m" in f else np.zeros((rows, K // 32))
    if dtype == L.Q8_0:
        return d, m, blk[..., f["q"]:].copy().view(np.int8).astype(np.int64)
    qs = blk[..., f["q"]:f["q"] + 16].astype(np.int64)
    q = np.concatenate([qs & 15, qs >> 4], axis=2)
    if "qh" in f:
        qh = blk[..., f["qh"]:f["qh"] + 4].copy().view("<u4").astype(np.int64)
        q |= ((qh >> np.arange(32)) & 1) << 4
    return d, m, q - BIAS[dtype]


def gemm64(dtype, w, rows, K, codes, scales, inv_s):
    """(y64, mag) [n][rows]: (1 / s_t) sum_b [d dx isum_b + m sx] in float64 and the same sum of magnitudes."""
    d, m, q = block_parts(dtype, w, rows, K)
    n = codes.shape[0]
    isum = np.einsum("rbk,tbk->trb", q, codes.reshape(n, -1, 32).astype(np.int64)).astype(np.float64)
    dx, sx = scales[..., 0].astype(np.float64)[:, None, :], scales[..., 1].astype(np.float64)[:, None, :]
    a, c = d[None] * dx * isum, m[None] * sx
    s = np.asarray(inv_s, np.float64)[:, None]
    return (a + c).sum(axis=2) * s, (np.abs(a) + np.abs(c)).sum(axis=2) * s


def bound(K, ks, mag):
    """one rounding per product d dx, multiply-add and slice sum, the cast of (1 / s_t) y: units of 2^-24 of mag"""
    return (K // 32 + ks + 3) * 2.0 ** -24 * mag + 1e-30


def definition_bound(dtype, w, rows, K, scales, inv_s):
    """half a code step per activation element against the block's sum of |w|, [n][rows]"""
    wabs = np.abs(G.decode_weights(dtype, w, rows, K)).reshape(rows, -1, 32).sum(axis=2)
    step = scales[..., 0].astype(np.float64) / 2 * np.asarray(inv_s, np.float64)[:, None]  # amax / 254 = dx / 2
    return (step @ wabs.T) * (1 + 2.0 ** -10)
