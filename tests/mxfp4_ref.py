"""Reference side of the MXFP4 tests: a numpy quantizer and dequantizer written from the format's
definition (include/xalm_hip.h), not from the C code.

A block is 17 bytes: e (E8M0), then 16 bytes, byte j holding element j in its low and element
j + 16 in its high nibble.  Code c has sign c >> 3 and magnitude {0, 0.5, 1, 1.5, 2, 3, 4, 6}[c & 7];
a weight is exactly value(c) * 2^(e - 127).  `quantize` works in float64, where every quantity it
forms is exact: |v| * 2^-E is a float32 significand under another exponent, and the nearest
magnitude is found by distance (a tie goes to the even code), not by thresholds as the C code does.

The oracle does not decode the format, so `oracle_from_xalm` hands it the rows dequantized to F32
(exact: every weight is a float32), as tests/gq2_ref.py does for the affine blocks.
"""
import numpy as np

from oracle import oracle as O
from xalm_amd import _lib as L

MAG = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
CODE_VALUES = np.concatenate([MAG, -MAG]).astype(np.float32)  # code 8 is -0
BLOCK = 17


def quantize(values):
    """float32 [..., n], n % 32 == 0 -> uint8 [..., n / 32 * 17]."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    if v.shape[-1] % 32 or not np.isfinite(v).all():
        raise ValueError("whole blocks of finite values")
    b = v.reshape(-1, 32)
    a = np.abs(b).astype(np.float64)
    amax = a.max(axis=1)
    # amax = m * 2^ex with m in [0.5, 1): floor(log2(amax)) = ex - 1, subnormals included
    _, ex = np.frexp(amax)
    E = np.clip(ex.astype(np.int64) - 1 - 2, -127, 127)
    t = np.ldexp(a, (-E)[:, None])
    dist = np.abs(t[:, :, None] - MAG[None, None, :])
    best = dist.min(axis=2, keepdims=True)
    # among the nearest magnitudes (two at a tie, adjacent codes) the even code
    odd = np.where(dist == best, np.arange(8)[None, None, :] % 2, 9)
    code = odd.argmin(axis=2).astype(np.uint8)
    code |= (np.signbit(b).astype(np.uint8) << 3)
    zero = amax == 0
    code[zero] = 0
    e = np.where(zero, 0, E + 127).astype(np.uint8)
    out = np.empty((b.shape[0], BLOCK), np.uint8)
    out[:, 0] = e
    out[:, 1:] = code[:, :16] | (code[:, 16:] << 4)
    return out.reshape(v.shape[:-1] + (v.shape[-1] // 32 * BLOCK,))


def parts(w):
    """Block bytes [..., k * 17] -> (e int64 [blocks], codes uint8 [blocks][32])."""
    blk = np.ascontiguousarray(w, dtype=np.uint8).reshape(-1, BLOCK)
    qs = blk[:, 1:]
    return blk[:, 0].astype(np.int64), np.concatenate([qs & 15, qs >> 4], axis=1)


def dequantize(w):
    """uint8 [..., k * 17] -> float32 [..., 32 k]; e = 255 (NaN) raises."""
    w = np.ascontiguousarray(w, dtype=np.uint8)
    e, c = parts(w)
    if (e == 255).any():
        raise ValueError("e = 255")
    v = np.ldexp(CODE_VALUES[c], (e - 127)[:, None].astype(np.int32)).astype(np.float32)
    return np.ascontiguousarray(v.reshape(w.shape[:-1] + (w.shape[-1] // BLOCK * 32,)))


def pack(e, codes):
    """Block bytes [rows][nb * 17] from e [rows][nb] and codes [rows][nb][32] (0..15): tensors no
    quantizer would produce (every code under every scale)."""
    c = np.asarray(codes, np.uint8)
    rows, nb = c.shape[:2]
    out = np.empty((rows, nb, BLOCK), np.uint8)
    out[:, :, 0] = np.asarray(e, np.uint8).reshape(rows, nb)
    out[:, :, 1:] = (c[..., :16] & 15) | ((c[..., 16:] & 15) << 4)
    return np.ascontiguousarray(out.reshape(rows, -1))


def mag_rows(w):
    """float64 [rows][n]: |w| per element, the scale the matvec's rounding follows."""
    return np.abs(dequantize(w).astype(np.float64))


LOOP_STRIDE = 37  # the token stride of the forward tests (tests/gq2_ref.py)


def loop_tokens(vocab, n=20):
    """BOS + n tokens at LOOP_STRIDE: the 21-token loop of the forward test.  make_mxfp4_fixtures.py
    asserts on the oracle that the six greedy steps after a 9-token prompt skip at most one token
    comparison under the top-two gap rule; if it fails, the stride changes, not the cap."""
    return [1] + [3 + (i * LOOP_STRIDE) % (vocab - 3) for i in range(n)]


def greedy_gap_count(om, toks, n_prompt=9, n_steps=6, gap=1e-3):
    """The oracle's own greedy continuation of toks[:n_prompt]: how many of its n_steps choices
    have a top-two gap above `gap` (the steps the GPU test compares)."""
    om.reset()
    for pos, tok in enumerate(toks[:n_prompt]):
        om.forward(tok, pos, L.OUTPUT_LOGITS if pos == n_prompt - 1 else L.HYDRATE_KV_CACHE)
    clear = 0
    for pos in range(n_prompt, n_prompt + n_steps):
        lg = om.logits()
        top2 = np.sort(lg)[-2:]
        clear += bool(top2[1] - top2[0] > gap)
        om.forward(O.sample_argmax(lg), pos)
    return clear


def model_tensors(xf):
    """(kind, layer, name) of every tensor Model::from_xalm loads."""
    cfg = xf.config()
    out = [(k, 0, n) for k, n in xf.global_tensors(bool(cfg.tie_word_embeddings)).items()]
    for layer in range(cfg.n_layers):
        out += [(k, layer, n) for k, n in xf.layer_tensors(layer).items()]
    return out


def oracle_from_xalm(xf, context=0, replace=None):
    """An OracleModel over the file's tensors, MXFP4 rows dequantized to F32.  replace: {name: block
    bytes [rows][...]} used in place of the file's."""
    cfg = xf.config(context)
    om = O.OracleModel(cfg)
    for kind, layer, name in model_tensors(xf):
        dt = xf.dtype(name)
        raw = np.ascontiguousarray(xf.raw(name))
        if replace and name in replace:
            raw = np.ascontiguousarray(replace[name]).reshape(-1)
        if dt == L.MXFP4:
            rows = xf.tensors[name].shape[0]
            om.set_tensor(kind, layer, L.F32, dequantize(raw.reshape(rows, -1)))
        else:
            om.set_tensor(kind, layer, dt, raw)
    return om


def lower_scales(w, by=20):
    """The matrix's values times 2^-by through the quantizer above: the same codes under e - by."""
    return quantize(np.ldexp(dequantize(w), -by).astype(np.float32))
