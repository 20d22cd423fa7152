"""numpy reference of the gguf K-quants XH_Q4_K / XH_Q6_K, written from the definitions in
include/xalm_hip.h: the decoders (the reference's quants.py pins them through tests/golden/kq_golden.npz)
and the project's quantizers (every float32 operation on its own, as xalm_synth.h has them)."""
import numpy as np

Q4_K, Q6_K = 26, 27
BYTES = {Q4_K: 144, Q6_K: 210}
F32 = np.float32


def _f16(b: np.ndarray) -> np.ndarray:
    """[..., 2] bytes -> float32 of the little-endian f16"""
    return np.ascontiguousarray(b).view(np.float16)[..., 0].astype(F32)


def q4k_fields(blk: np.ndarray):
    """[nb, 144] uint8 -> d, dmin [nb], sc, mn [nb, 8] (ints), q [nb, 256] (ints)"""
    s = blk[:, 4:16].astype(np.int32)
    sc = np.empty((blk.shape[0], 8), np.int32)
    mn = np.empty_like(sc)
    for j in range(8):
        if j < 4:
            sc[:, j] = s[:, j] & 63
            mn[:, j] = s[:, j + 4] & 63
        else:
            sc[:, j] = (s[:, j + 4] & 15) | ((s[:, j - 4] >> 6) << 4)
            mn[:, j] = (s[:, j + 4] >> 4) | ((s[:, j] >> 6) << 4)
    qs = blk[:, 16:144].astype(np.int32).reshape(-1, 4, 32)
    q = np.stack([qs & 15, qs >> 4], axis=2).reshape(-1, 256)  # element 64g + 32 hi + l
    return _f16(blk[:, 0:2]), _f16(blk[:, 2:4]), sc, mn, q


def q6k_fields(blk: np.ndarray):
    """[nb, 210] uint8 -> d [nb], sc [nb, 16] (ints), q [nb, 256] (ints 0..63)"""
    ql = blk[:, 0:128].astype(np.int32)
    qh = blk[:, 128:192].astype(np.int32)
    q = np.empty((blk.shape[0], 256), np.int32)
    l = np.arange(32)
    for h in range(2):
        for k in range(4):
            lo = (ql[:, 64 * h + 32 * (k & 1) + l] >> (4 * (k >> 1))) & 15
            hi = (qh[:, 32 * h + l] >> (2 * k)) & 3
            q[:, 128 * h + 32 * k + l] = lo | (hi << 4)
    return _f16(blk[:, 208:210]), blk[:, 192:208].view(np.int8).astype(np.int32), q


def dequantize(dtype: int, blocks: np.ndarray) -> np.ndarray:
    """uint8 [..., k * bytes] -> float32 [..., 256 k]"""
    b = np.ascontiguousarray(blocks, dtype=np.uint8)
    blk = b.reshape(-1, BYTES[dtype])
    with np.errstate(all="ignore"):
        if dtype == Q4_K:
            d, dmin, sc, mn, q = q4k_fields(blk)
            D = np.repeat(d[:, None] * sc.astype(F32), 32, axis=1)     # exact
            M = np.repeat(dmin[:, None] * mn.astype(F32), 32, axis=1)  # exact
            # (D q) is exact, so the float32 difference is fmaf(D, q, -M): one rounding
            out = (D * q.astype(F32) - M).astype(F32)
        else:
            d, sc, q = q6k_fields(blk)
            out = (np.repeat(d[:, None] * sc.astype(F32), 16, axis=1) * (q - 32).astype(F32)).astype(F32)
    return out.reshape(b.shape[:-1] + (b.shape[-1] // BYTES[dtype] * 256,))


def terms(dtype: int, blocks: np.ndarray) -> np.ndarray:
    """|d_eff q| + |m_eff| of every weight (Q6_K: |d sc (q - 32)|), float64: the magnitude of the
    matvec bar"""
    blk = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, BYTES[dtype])
    if dtype == Q4_K:
        d, dmin, sc, mn, q = q4k_fields(blk)
        D = np.repeat(d.astype(np.float64)[:, None] * sc, 32, axis=1)
        M = np.repeat(dmin.astype(np.float64)[:, None] * mn, 32, axis=1)
        t = np.abs(D * q) + np.abs(M)
    else:
        d, sc, q = q6k_fields(blk)
        t = np.abs(np.repeat(d.astype(np.float64)[:, None] * sc, 16, axis=1) * (q - 32))
    return t.reshape(blocks.shape[:-1] + (-1,))


def _to_f16(x: np.ndarray) -> np.ndarray:
    """float32 -> f16 by round-to-nearest-even, saturating at 65504 (xs_to_f16)"""
    return np.minimum(x, F32(65504.0)).astype(np.float16)


def _field(a: np.ndarray, d: np.ndarray, cap: int) -> np.ndarray:
    """min(cap, floor(a / d + 0.5)), 0 where d == 0 (xs_kq_field)"""
    with np.errstate(all="ignore"):
        t = (a / d).astype(F32)
        r = np.floor((t + F32(0.5)).astype(F32))
    r = np.where(d == 0, F32(0), np.minimum(r, F32(cap)))
    return r.astype(np.int32)


def _codes(t: np.ndarray, add: float, top: int, live: np.ndarray) -> np.ndarray:
    r = np.floor((t + F32(add)).astype(F32))
    return np.where(live, np.clip(r, 0, top), 0).astype(np.int32)


def quantize(dtype: int, values: np.ndarray) -> np.ndarray:
    """float32 [..., 256 k] -> uint8 [..., k * bytes]: the project's quantizer"""
    v = np.ascontiguousarray(values, dtype=F32)
    sb = v.reshape(-1, 256)
    nb = sb.shape[0]
    out = np.zeros((nb, BYTES[dtype]), np.uint8)
    with np.errstate(all="ignore"):
        if dtype == Q4_K:
            g = sb.reshape(nb, 8, 32)
            lo = np.minimum(g.min(axis=2), F32(0))
            a = ((g.max(axis=2) - lo).astype(F32) / F32(15)).astype(F32)
            b = (F32(0) - lo).astype(F32)
            dh = _to_f16((a.max(axis=1) / F32(63)).astype(F32))
            mh = _to_f16((b.max(axis=1) / F32(63)).astype(F32))
            d, dmin = dh.astype(F32), mh.astype(F32)
            sc = _field(a, d[:, None], 63)
            mn = _field(b, dmin[:, None], 63)
            D = (d[:, None] * sc.astype(F32)).astype(F32)
            M = (dmin[:, None] * mn.astype(F32)).astype(F32)
            t = ((g + M[:, :, None]).astype(F32) / D[:, :, None]).astype(F32)
            q = _codes(t, 0.5, 15, np.broadcast_to((D != 0)[:, :, None], t.shape)).reshape(nb, 256)
            out[:, 0:2] = dh.view(np.uint8).reshape(nb, 2)
            out[:, 2:4] = mh.view(np.uint8).reshape(nb, 2)
            for j in range(4):
                out[:, 4 + j] = sc[:, j] | ((sc[:, j + 4] >> 4) << 6)
                out[:, 8 + j] = mn[:, j] | ((mn[:, j + 4] >> 4) << 6)
                out[:, 12 + j] = (sc[:, j + 4] & 15) | ((mn[:, j + 4] & 15) << 4)
            q4 = q.reshape(nb, 4, 2, 32)
            out[:, 16:144] = (q4[:, :, 0, :] | (q4[:, :, 1, :] << 4)).reshape(nb, 128)
        else:
            g = sb.reshape(nb, 16, 16)
            a = (np.abs(g).max(axis=2) / F32(31)).astype(F32)
            dh = _to_f16((a.max(axis=1) / F32(127)).astype(F32))
            d = dh.astype(F32)
            sc = _field(a, d[:, None], 127)
            D = (d[:, None] * sc.astype(F32)).astype(F32)
            t = (g / D[:, :, None]).astype(F32)
            q = _codes(t, 32.5, 63, np.broadcast_to((D != 0)[:, :, None], t.shape)).reshape(nb, 2, 4, 32)
            lo4, hi2 = q & 15, q >> 4
            for h in range(2):
                out[:, 64 * h:64 * h + 32] = lo4[:, h, 0] | (lo4[:, h, 2] << 4)
                out[:, 64 * h + 32:64 * h + 64] = lo4[:, h, 1] | (lo4[:, h, 3] << 4)
                out[:, 128 + 32 * h:160 + 32 * h] = hi2[:, h, 0] | (hi2[:, h, 1] << 2) | (hi2[:, h, 2] << 4) | (hi2[:, h, 3] << 6)
            out[:, 192:208] = sc.astype(np.int8).view(np.uint8)
            out[:, 208:210] = dh.view(np.uint8).reshape(nb, 2)
    return out.reshape(v.shape[:-1] + (v.shape[-1] // 256 * BYTES[dtype],))


def error_bound(dtype: int, blocks: np.ndarray) -> np.ndarray:
    """The per-element bound xalm_hip.h states for the quantizer, from the blocks it wrote (float64)"""
    blk = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, BYTES[dtype])
    if dtype == Q4_K:
        d, dmin, sc, _, _ = q4k_fields(blk)
        d, dmin = d.astype(np.float64)[:, None], dmin.astype(np.float64)[:, None]
        b = np.repeat(np.maximum(d * sc / 2, 8 * d + dmin), 32, axis=1) * (1 + 2.0 ** -16) + 2.0 ** -14
    else:
        d, sc, _ = q6k_fields(blk)
        d = d.astype(np.float64)[:, None]
        b = np.repeat(np.maximum(d * np.abs(sc) / 2, 17 * d), 16, axis=1) * (1 + 2.0 ** -16) + 2.0 ** -13
    return b.reshape(blocks.shape[:-1] + (-1,))


def random_blocks(dtype: int, n_blocks: int, rng: np.random.Generator, scale_exp=(-12, 2)) -> np.ndarray:
    """Blocks of random bytes with the f16 scale fields forced finite (a random sign, exponent in
    scale_exp, mantissa): every such block is valid."""
    blk = rng.integers(0, 256, size=(n_blocks, BYTES[dtype]), dtype=np.uint8)
    def scales(n):
        e = rng.integers(scale_exp[0] + 15, scale_exp[1] + 15, size=n).astype(np.uint16)
        h = (rng.integers(0, 2, size=n).astype(np.uint16) << 15) | (e << 10) | rng.integers(0, 1024, size=n).astype(np.uint16)
        return h.view(np.uint8).reshape(n, 2)
    if dtype == Q4_K:
        blk[:, 0:2] = scales(n_blocks)
        blk[:, 2:4] = scales(n_blocks)
    else:
        blk[:, 208:210] = scales(n_blocks)
    return blk
