"""Reference side of the affine / 5-bit block tests (Q4_1 / Q5_0 / Q5_1).

The oracle decodes Q8_0 and Q4_0 only, so these tests hand it the blocks DEQUANTIZED: `dequant`
restates quants.py ``dequantize_blocks`` in numpy float32 (d*q exact, then one rounding of + m,
i.e. fmaf(d, q, m)) and is pinned bit for bit against quants.py's own floats in
tests/golden/gq2_golden.npz (tests/test_gq2_cpu.py).  `oracle_from_xalm` builds an OracleModel over
those float32 rows (norm vectors as stored), which is exact: the oracle then runs the reference
forward over exactly the dequantized weights.
"""
import numpy as np

from oracle import oracle as O
from xalm_amd import _lib as L

TYPES = {"q4_1": L.Q4_1, "q5_0": L.Q5_0, "q5_1": L.Q5_1}
HAS_M = {L.Q4_1: True, L.Q5_0: False, L.Q5_1: True}
HAS_QH = {L.Q4_1: False, L.Q5_0: True, L.Q5_1: True}


def parts(dtype, w):
    """Block bytes [rows][n/32 * block bytes] -> (d, m, q) as float32 [rows * n/32][1 | 32]:
    value = d * q + m, q already less the format's offset (Q5_0: q - 16)."""
    blk = np.ascontiguousarray(w).reshape(-1, L.GQ_BLOCK_BYTES[dtype])
    d = blk[:, 0:2].copy().view(np.float16).astype(np.float32)
    o = 2
    m = np.zeros_like(d)
    if HAS_M[dtype]:
        m = blk[:, o:o + 2].copy().view(np.float16).astype(np.float32)
        o += 2
    hi = np.zeros((blk.shape[0], 32), np.uint8)
    if HAS_QH[dtype]:
        qh = blk[:, o:o + 4].copy().view("<u4")
        hi = ((qh >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8)
        o += 4
    qs = blk[:, o:]
    q = np.concatenate([qs & 15, qs >> 4], axis=1) | (hi << 4)
    q = q.astype(np.float32) - np.float32(16 if dtype == L.Q5_0 else 0)
    return d, m, q


def pack(dtype, d, m, q):
    """Block bytes in the file layout from f16 d, m [rows][nb] and codes q [rows][nb][32] (0..15 /
    0..31): tensors no quantizer would produce (e.g. every fifth bit set)."""
    q = np.asarray(q, np.uint8)
    rows, nb = q.shape[:2]
    cols = [np.asarray(d, np.float16).reshape(rows, nb, 1).view(np.uint8)]
    if HAS_M[dtype]:
        cols.append(np.asarray(m, np.float16).reshape(rows, nb, 1).view(np.uint8))
    if HAS_QH[dtype]:
        qh = ((q >> 4).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(axis=-1, dtype=np.uint32)
        cols.append(qh.astype("<u4").reshape(rows, nb, 1).view(np.uint8))
    cols.append((q[..., :16] & 15) | ((q[..., 16:] & 15) << 4))
    return np.ascontiguousarray(np.concatenate(cols, axis=-1).reshape(rows, -1))


def dequant(dtype, w):
    """float32 [rows][n]: the converter's value of every weight."""
    d, m, q = parts(dtype, w)
    v = d * q
    if HAS_M[dtype]:
        v = v + m
    return np.ascontiguousarray(v.reshape(np.asarray(w).shape[0], -1), dtype=np.float32)


def mag_rows(dtype, w):
    """float64 [rows][n]: |d q| + |m| per element, the scale the matvec's rounding follows (the
    affine kernel sums d * sum(q x) and m * sum(x) separately)."""
    d, m, q = parts(dtype, w)
    v = np.abs(d.astype(np.float64) * q) + np.abs(m.astype(np.float64))
    return v.reshape(np.asarray(w).shape[0], -1)


def positive_case(dtype, n, d):
    """All-positive weights in [1, 1.1) (m >= 1 dominates every block, d*q never cancels it)
    against x ~ N(0, 1): (block bytes, x).  x is signed on purpose: against x of one sign the
    result is a sum of n same-sign terms of size mag / n, and the f32 reference matvec alone misses
    the bar at n = 4096 (its error measured at 1.07 - 1.22 x the bar on the CPU); with signed x the
    reference stays far inside (tests/test_gq2_cpu.py asserts it), while a dropped m * sum(x) still
    moves the result by about sqrt(n), thousands of times the bar."""
    rng = np.random.default_rng(n + dtype)
    wf = rng.uniform(1.0, 1.1, (d, n)).astype(np.float32)
    x = rng.standard_normal(n).astype(np.float32)
    return L.quantize_blocks(dtype, wf), x


POSITIVE_SHAPES = [(512, 96), (4096, 64)]
LOOP_STRIDE = 37  # the token stride of test_forward_on_converter_blocks (tests/test_gq_gpu.py)


def loop_tokens(vocab, n=20):
    """BOS + n tokens at LOOP_STRIDE: the 21-token loop of the forward tests.  The stride is
    chosen so the greedy steps after a 9-token prompt skip at most one token comparison per
    fixture under the top-two gap rule (tests/test_gq2_cpu.py checks it on the oracle)."""
    return [1] + [3 + (i * LOOP_STRIDE) % (vocab - 3) for i in range(n)]


def model_tensors(xf):
    """(kind, layer, name) of every tensor Model::from_xalm loads."""
    cfg = xf.config()
    out = [(k, 0, n) for k, n in xf.global_tensors(bool(cfg.tie_word_embeddings)).items()]
    for layer in range(cfg.n_layers):
        out += [(k, layer, n) for k, n in xf.layer_tensors(layer).items()]
    return out


def oracle_from_xalm(xf, context=0):
    cfg = xf.config(context)
    om = O.OracleModel(cfg)
    for kind, layer, name in model_tensors(xf):
        dt = xf.dtype(name)
        raw = np.ascontiguousarray(xf.raw(name))
        if dt in TYPES.values():
            rows = xf.tensors[name].shape[0]
            om.set_tensor(kind, layer, L.F32, dequant(dt, raw.reshape(rows, -1)))
        else:
            om.set_tensor(kind, layer, dt, raw)
    return om
