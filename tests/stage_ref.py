"""Float64 reference of one decoder layer, stage by stage, and the bar of every stage.

One decode step of a one-layer model is five fused launches (GemvRole, xalm_amd/csrc/ctx.h):
QKV, attention + Wo, GLU (W1/W3), W2, LOGITS.  Each stage is computed here in float64 from the
OBSERVED output of the stage before it (teacher forcing), so every bar is a one-stage bar and an
error cannot hide behind, or be blamed on, the stages around it:

    x0      the embedding row, decoded on the host (exact)
    QKV     xn = rmsnorm(x0); q, k, v = W xn; clip; RoPE on q and k (the frequency table exactly as
            xh_create builds it: f32, host libm).  q compared in f32, the ring rows k, v in f16.
    ATTN    softmax attention of the observed q over the observed ring, x1 = x0 + Wo att.  x1 is
            observed on a second context whose W2 is zeros of the same dtype (x1 + 0).
    GLU     hb = act(W1 xn1) * (W3 xn1), xn1 = rmsnorm(observed x1)
    W2      x2 = observed x1 + W2 (observed hb)
    LOGITS  Wcls rmsnorm(observed x2); one greedy step returns sample_argmax of the observed logits.

Bars.  They are derived from the project's own constants, not tuned; `mag` is the float64
sum |w| |input| of the row, plus |residual| where one is added (affine gguf types: |d q| + |m| for
|w|, as tests/gq2_ref.py):
    matvec output        2e-6 mag + 1e-7                       (tests/test_ops_gpu.py)
    clip                 1-Lipschitz: the bar passes through
    RoPE pair            the rotated bars, |c| b0 + |s| b1, plus 4e-6 max(|v0|, |v1|)   (test_rope)
    GLU                  1.13 |u| bg + |act(g)| bu + 2e-7 |hb|  (1.13 bounds |SiLU'| and |GELU'|)
    f16 ring rows        the f32 bar plus one f16 ulp, |ref| 2^-10 + 2^-24
    attention into Wo    |wo| @ min(bar_att, 2e-5) + 2e-6 mag + 1e-7   (bar_att per attention element:
                         tests/attn_ref.py; 2e-5: test_mha's flat bar, so the term is never looser than it was)

Oracle headroom.  tests/test_stages_cpu.py composes the same stages from the CPU oracle's f32 ops
and requires them under every bar with at least 4x headroom (the GPU sums in another order).
Worst err / bar of the f32 oracle over the whole sweep (252 cases), measured on the CPU:
    q 0.094   x1 0.007   hb 0.084   x2 0.157   logits 0.109   (headroom 6x and more)
(x1: 0.004 under the flat 2e-5 sum|wo| this term replaces.  At this sweep's 41 slots bar_att is
0.6 to 2.4 times smaller than 2e-5 by element: larger than 2e-5 for some elements at head_dim 128,
where the scores are large, hence the minimum.)
    k 0.493   v 0.494
k and v are the f16 rounding itself: up to half an ulp in every correct evaluation, half of the
bar's one-ulp term whatever the summation order, so their ratio approaches 1/2 by construction;
the 4x is asked of the f32 part beside it, (ulp / 2 + b32 / 4) / (ulp + b32) <= 1 / 2.  No stage
fell short, so no bar is widened, and none is calibrated from GPU output.
"""
import ctypes
import ctypes.util

import numpy as np

from oracle import oracle as O
from xalm_amd import _lib as L

import attn_ref as AR
import stage_cases as SC

STAGES = ("q", "k", "v", "x1_fused", "x1_split", "hb", "x2", "logits")
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]

SEED = {L.EMBED: 11, L.WCLS: 12, L.FINAL_NORM: 13, L.WQ: 100, L.WK: 101, L.WV: 102, L.WO: 103, L.W1: 104, L.W2: 105,
        L.W3: 106, L.ATTN_NORM: 300, L.FFN_NORM: 400}
KV_SEED = (900, 901)
MATRICES = (L.WQ, L.WK, L.WV, L.WO, L.W1, L.W2, L.W3, L.WCLS)


def shapes(c):
    q_dim, kv_dim = c.heads * c.head_dim, c.kv_heads * c.head_dim
    return {L.EMBED: (c.vocab, c.dim), L.WCLS: (c.vocab, c.dim), L.FINAL_NORM: (1, c.dim), L.ATTN_NORM: (1, c.dim),
            L.FFN_NORM: (1, c.dim), L.WQ: (q_dim, c.dim), L.WK: (kv_dim, c.dim), L.WV: (kv_dim, c.dim),
            L.WO: (c.dim, q_dim), L.W1: (c.hidden, c.dim), L.W2: (c.dim, c.hidden), L.W3: (c.hidden, c.dim)}


def tensor_specs(c, wdt):
    """[(kind, dtype, seed, mean, std)]: matrices of std 0.7 / sqrt(inputs), so every activation
    stays of order 1 at every width (q about 0.7: test_mha's regime); norms 1 +- 0.01."""
    edt = wdt if c.tied else L.F16
    out = [(L.EMBED, edt, SEED[L.EMBED], 0.0, 1.0)]
    for kind in (L.FINAL_NORM, L.ATTN_NORM, L.FFN_NORM):
        out.append((kind, c.norm_dt, SEED[kind], 1.0, 0.01))
    for kind in MATRICES:
        if kind == L.WCLS and c.tied:
            continue
        out.append((kind, wdt, SEED[kind], 0.0, 0.7 / np.sqrt(shapes(c)[kind][1])))
    return out


def host_tensor(rows, cols, dt, seed, mean, std):
    """The host copy of xh_upload_synthetic's tensor in the upload layout.  Q8 (int8 x 0.01) has no
    synthetic fill: seeded integers of about the same spread, uploaded from the host."""
    if dt == L.Q8:
        r = max(1, int(round(100.0 * std * 1.7320508)))
        return np.random.default_rng(seed).integers(-r, r + 1, (rows, cols), dtype=np.int8)
    if dt in L.GQ_BLOCK_BYTES:
        vals = np.asarray(O.synthetic(rows, cols, L.F32, seed, mean, std), np.float32).reshape(rows, cols)
        return L.quantize_blocks(dt, vals)
    return np.asarray(O.synthetic(rows, cols, dt, seed, mean, std)).reshape(rows, cols)


def host_weights(c, wdt):
    """{kind: (dtype, array [rows][...])} of every tensor of the case."""
    sh = shapes(c)
    return {kind: (dt, host_tensor(sh[kind][0], sh[kind][1], dt, seed, mean, std))
            for kind, dt, seed, mean, std in tensor_specs(c, wdt)}


def zero_matrix(dt, rows, cols):
    """A matrix whose every weight decodes to 0: zero floats, fp8 / int8 code 0, quantized zeros."""
    if dt in L.GQ_BLOCK_BYTES:
        return L.quantize_blocks(dt, np.zeros((rows, cols), np.float32))
    return np.zeros((rows, cols), {L.F32: np.float32, L.F16: np.uint16, L.BF16: np.uint16}.get(dt, np.uint8))


_TABLES = {}


def _byte_table(dt):
    if dt not in _TABLES:
        codes = np.arange(256, dtype=np.uint8)
        src = codes.view(np.int8) if dt == L.Q8 else codes
        _TABLES[dt] = np.array([O.decode(dt, src, i) for i in range(256)], dtype=np.float64)
    return _TABLES[dt]


def decode64(dt, raw, cols):
    """(value, magnitude) in float64 [rows][cols]: every weight exactly as the format defines it,
    and |d q| + |m| (= |value| except for the affine block types)."""
    raw = np.ascontiguousarray(raw)
    rows = raw.shape[0]
    if dt == L.F32:
        w = raw.view(np.float32).astype(np.float64)
    elif dt == L.F16:
        w = raw.view(np.float16).astype(np.float64)
    elif dt == L.BF16:
        w = (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    elif dt in (L.F8_E4M3, L.F8_E5M2, L.Q8):
        w = _byte_table(dt)[raw.view(np.uint8)]
    else:
        blk = raw.reshape(-1, L.GQ_BLOCK_BYTES[dt])
        d = blk[:, 0:2].copy().view(np.float16).astype(np.float64)
        o = 2
        m = np.zeros_like(d)
        if dt in (L.Q4_1, L.Q5_1):
            m = blk[:, o:o + 2].copy().view(np.float16).astype(np.float64)
            o += 2
        if dt == L.Q8_0:
            q = blk[:, o:].view(np.int8).astype(np.float64)
        else:
            hi = np.zeros((blk.shape[0], 32), np.uint8)
            if dt in (L.Q5_0, L.Q5_1):
                qh = blk[:, o:o + 4].copy().view("<u4")
                hi = ((qh >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8)
                o += 4
            qs = blk[:, o:]
            q = (np.concatenate([qs & 15, qs >> 4], axis=1) | (hi << 4)).astype(np.float64)
            q -= {L.Q4_0: 8.0, L.Q5_0: 16.0}.get(dt, 0.0)
        return (d * q + m).reshape(rows, cols), (np.abs(d * q) + np.abs(m)).reshape(rows, cols)
    w = w.reshape(rows, cols)
    return w, np.abs(w)


def norm64(dt, raw):
    return decode64(dt, np.asarray(raw).reshape(1, -1), np.asarray(raw).size)[0][0]


def f16_to_64(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def rmsnorm64(x, w, eps):
    x = np.asarray(x, np.float64)
    return x / np.sqrt(np.mean(x * x) + np.float64(np.float32(eps))) * w


def act64(act, g):
    if act == L.ACT_SILU:
        return g / (1.0 + np.exp(-g))
    return 0.5 * g * (1.0 + np.tanh(np.float64(np.float32(0.797885)) * (g + np.float64(np.float32(0.044715)) * g ** 3)))


def rope_cs(c, pos):
    """(cos, sin) per pair of a head in float64, of the f32 angle the device forms: freq[j] =
    1 / powf(theta, j / rotary_dim) with the host libm (0 past rotary_dim), val = (float)pos * freq."""
    theta = np.float32(10000.0)
    val = np.zeros(c.head_dim // 2, np.float32)
    for j in range(0, c.head_dim, 2):
        if j < c.rotary:
            freq = np.float32(1.0) / np.float32(_libm.powf(theta, np.float32(j) / np.float32(c.rotary)))
            val[j // 2] = np.float32(pos) * freq
    return np.cos(val.astype(np.float64)), np.sin(val.astype(np.float64))


def matvec(wd, wm, x, resid=None):
    """(W x [+ resid], bar) of one matvec in float64."""
    x = np.asarray(x, np.float64)
    y = wd @ x
    mag = wm @ np.abs(x)
    if resid is not None:
        y = y + resid
        mag = mag + np.abs(resid)
    return y, 2e-6 * mag + 1e-7


def rope_bar(c, v, b, cs):
    """v [heads * head_dim] clipped values with bars b -> (rotated, bars)."""
    cos, sin = (np.tile(t, v.size // c.head_dim) for t in cs)
    v0, v1, b0, b1 = v[0::2], v[1::2], b[0::2], b[1::2]
    extra = 4e-6 * np.maximum(np.abs(v0), np.abs(v1))
    out, bar = np.empty_like(v), np.empty_like(b)
    out[0::2], out[1::2] = v0 * cos - v1 * sin, v0 * sin + v1 * cos
    bar[0::2] = np.abs(cos) * b0 + np.abs(sin) * b1 + extra
    bar[1::2] = np.abs(sin) * b0 + np.abs(cos) * b1 + extra
    return out, bar


class Obs:
    """What one decode step left: q [q_dim] f32, k_row / v_row [kv_dim] f16 bits, x1 {fuse: [dim]},
    hb [hidden], x2 [dim], logits [vocab], greedy (the next token of one greedy step, or None)."""
    q = k_row = v_row = x1 = hb = x2 = logits = greedy = None


def check_stages(c, wdt, W, obs, pos=SC.HIST):
    """{stage: worst err / bar} of the observation against the float64 stages.  W: host_weights."""
    eps, q_dim, kv_dim = 1e-5, c.heads * c.head_dim, c.kv_heads * c.head_dim
    dec = {k: decode64(dt, a, shapes(c)[k][1]) for k, (dt, a) in W.items() if k in MATRICES}
    nrm = {k: norm64(*W[k]) for k in (L.ATTN_NORM, L.FFN_NORM, L.FINAL_NORM)}
    edt, emb = W[L.EMBED]
    x0 = decode64(edt, emb[SC.TOKEN:SC.TOKEN + 1], c.dim)[0][0]
    ratio = {}

    # QKV: rmsnorm, matvec, clip, rope, f16 ring rows
    xn = rmsnorm64(x0, nrm[L.ATTN_NORM], eps)
    cs = rope_cs(c, pos)
    out = {}
    for name, kind in (("q", L.WQ), ("k", L.WK), ("v", L.WV)):
        y, b = matvec(*dec[kind], xn)
        y = np.clip(y, -np.float64(np.float32(c.clip)), np.float64(np.float32(c.clip)))
        out[name] = rope_bar(c, y, b, cs) if name != "v" else (y, b)
    ratio["q"] = float(np.max(np.abs(obs.q - out["q"][0]) / out["q"][1]))
    for name, row in (("k", obs.k_row), ("v", obs.v_row)):
        ref, b = out[name]
        ratio[name] = float(np.max(np.abs(f16_to_64(row) - ref) / (b + np.abs(ref) * 2.0 ** -10 + 2.0 ** -24)))

    # attention over the observed ring (history + the new row) from the observed q, then Wo
    kb = np.concatenate([f16_to_64(history(c, 0)), f16_to_64(obs.k_row)[None]])
    vb = np.concatenate([f16_to_64(history(c, 1)), f16_to_64(obs.v_row)[None]])
    att, bar_att, _ = AR.attention64(kb, vb, obs.q, c.head_dim, kb.shape[0], c.heads, c.kv_heads)
    x1, b = matvec(*dec[L.WO], att, x0)
    b = b + dec[L.WO][1] @ np.minimum(bar_att, 2e-5)
    for fuse, name in ((1, "x1_fused"), (0, "x1_split")):
        if fuse in obs.x1:
            ratio[name] = float(np.max(np.abs(obs.x1[fuse] - x1) / b))

    # GLU from the observed x1 (the one the full model's own launches produced)
    x1o = obs.x1[max(obs.x1)].astype(np.float64)
    xn1 = rmsnorm64(x1o, nrm[L.FFN_NORM], eps)
    (g, bg), (u, bu) = matvec(*dec[L.W1], xn1), matvec(*dec[L.W3], xn1)
    hb = act64(c.act, g) * u
    ratio["hb"] = float(np.max(np.abs(obs.hb - hb) / (1.13 * np.abs(u) * bg + np.abs(act64(c.act, g)) * bu + 2e-7 * np.abs(hb))))

    # W2 from the observed hb and x1
    x2, b = matvec(*dec[L.W2], obs.hb, x1o)
    ratio["x2"] = float(np.max(np.abs(obs.x2 - x2) / b))

    # LOGITS from the observed x2; the greedy step is exact on the observed logits
    wc = decode64(edt, emb, c.dim) if c.tied else dec[L.WCLS]
    lg, b = matvec(*wc, rmsnorm64(obs.x2, nrm[L.FINAL_NORM], eps))
    ratio["logits"] = float(np.max(np.abs(obs.logits - lg) / b))
    if obs.greedy is not None:
        assert obs.greedy == O.sample_argmax(obs.logits), ("greedy", obs.greedy, O.sample_argmax(obs.logits))
    return ratio


def history(c, which):
    """The synthetic K (0) / V (1) history, f16 bits [HIST][kv_dim] (xh_kv_fill_synthetic's rows)."""
    return np.asarray(O.synthetic(SC.HIST, c.kv_heads * c.head_dim, L.F16, KV_SEED[which], 0.0, 1.0)).reshape(SC.HIST, -1)


# -- the same stages from the CPU oracle's f32 ops (tests/test_stages_cpu.py) ----------------------
def _omatmul(x, dt, raw, n, d):
    if dt in (L.Q4_1, L.Q5_0, L.Q5_1):  # the oracle decodes no affine / 5-bit blocks: their f32 values
        w = decode64(dt, raw, n)[0].astype(np.float32)
        return O.matmul(x, w, L.F32, n, d)
    return O.matmul(x, raw, dt, n, d)


def oracle_observe(c, wdt, W, pos=SC.HIST):
    """Obs of one step evaluated with the oracle's f32 ops (O.rmsnorm, O.matmul, O.rope, O.mha),
    each stage fed what the stage before it produced here."""
    f32 = np.float32
    sh = shapes(c)
    mm = lambda x, kind: _omatmul(x, W[kind][0], W[kind][1], sh[kind][1], sh[kind][0])
    nw = lambda kind: np.ascontiguousarray(W[kind][1]).reshape(-1)
    edt, emb = W[L.EMBED]
    x0 = decode64(edt, emb[SC.TOKEN:SC.TOKEN + 1], c.dim)[0][0].astype(f32)
    o = Obs()
    xn = O.rmsnorm(x0, nw(L.ATTN_NORM), c.norm_dt, 1e-5)
    clip = lambda v: np.clip(v, -f32(c.clip), f32(c.clip)).astype(f32)
    o.q = O.rope(clip(mm(xn, L.WQ)), c.head_dim, pos, 10000.0, c.rotary)
    k = O.rope(clip(mm(xn, L.WK)), c.head_dim, pos, 10000.0, c.rotary)
    o.k_row = k.astype(np.float16).view(np.uint16)
    o.v_row = clip(mm(xn, L.WV)).astype(np.float16).view(np.uint16)
    kb = np.zeros((SC.MSL, k.size), np.uint16)
    vb = np.zeros_like(kb)
    kb[:SC.HIST], vb[:SC.HIST] = history(c, 0), history(c, 1)
    kb[SC.HIST], vb[SC.HIST] = o.k_row, o.v_row
    att = O.mha(kb, vb, o.q, c.head_dim, SC.HIST + 1, SC.MSL, c.heads, c.kv_heads)
    x1 = (x0 + mm(att, L.WO)).astype(f32)
    o.x1 = {1: x1}
    xn1 = O.rmsnorm(x1, nw(L.FFN_NORM), c.norm_dt, 1e-5)
    g, u = mm(xn1, L.W1), mm(xn1, L.W3)
    if c.act == L.ACT_SILU:
        a = (g / (f32(1) + np.exp(-g, dtype=f32))).astype(f32)
    else:
        a = (f32(0.5) * g * (f32(1) + np.tanh(f32(0.797885) * (g + f32(0.044715) * g * g * g), dtype=f32))).astype(f32)
    o.hb = (a * u).astype(f32)
    o.x2 = (x1 + mm(o.hb, L.W2)).astype(f32)
    xn2 = O.rmsnorm(o.x2, nw(L.FINAL_NORM), c.norm_dt, 1e-5)
    o.logits = _omatmul(xn2, *(W[L.EMBED] if c.tied else W[L.WCLS]), c.dim, c.vocab)
    return o
