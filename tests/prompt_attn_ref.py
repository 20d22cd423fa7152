"""Float64 reference, bar, arithmetic mutants and case table of the prompt-pass attention
(xh_op_prompt_attn / xh_op_prompt_attn_ring: prefill_fa_kernel, prefill_fa2_kernel,
prefill_fa2_ring_kernel, prefill_fa_merge_kernel, prefill_ring_commit_kernel).

Definition (src/infer.cpp:279-301, :338, :608-613), per query row t and head h, KV head g = h // qpk:
  causal  s_j = (q . K[j][g]) * float(1 / sqrtf(hd)) over slots j <= pos0 + t, p = softmax(s) with the
          max subtracted, out = sum_j p_j V[j][g].
  ring    the row sees the sink slots r = 0, 1 (scored against sink_ver[t][r], values v_ring[r]) and
          the virtual rows u in [t + 1, W + t], W = max_seq_len - 2: u < W is ring slot
          2 + (hoff + u) % W with hoff = (p0 - 2) % W, u >= W is staging row u - W.

Bar, per output element d ("Prompt attention"):
  bar = (2 ds + 4e-6) * sum_j p_j |V[j][d]| + 1e-7,   ds = 5e-7 * max_j sum_k |q_k K[j][k]| * scale
(ds: the 2^-22 split of q and the f32 sum of exact products; a score error e moves a softmax
weight by at most 2 e relative; 2e-6 for __expf in the numerator and again in the sum).

Mutants: the same evaluation with the lo half of q (split under the row's power-of-two scale, as
fa2_body) or of p dropped from the MFMA operands, which is what a kernel missing one of its `lo`
MFMAs computes.  The sink scores are formed by the merge kernel from the f32 q and the running
sum from the f32 p, so neither is touched.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

Q_SCALE, KV_STD = 0.5, 1.0
VARIANTS = ("f64", "f32", "q_hi_only", "p_hi_only")


def f16_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).astype(np.float16).view(np.uint16)


def f16_vals(bits, dtype=np.float64):
    return np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16).astype(dtype)


def attn_scale(hd):
    return np.float32(1.0) / np.sqrt(np.float32(hd))  # src/infer.cpp:338


def q_hi(q):
    """The hi half of q's f16 split: rows [..., hd] scaled by 2^(15 - ex), frexp(max |q|) = (f, ex)."""
    mx = np.abs(q).max(axis=-1, keepdims=True)
    ex = np.frexp(np.where(mx > 0, mx, 1.0))[1]
    sc = np.where(mx > 0, np.exp2(15.0 - ex), 1.0)
    return (q * sc).astype(np.float32).astype(np.float16).astype(q.dtype) / sc


def _head(q, K, V, vis, xk, xv, scale, variant):
    """One head.  q [n][hd]; K, V [S][hd] with vis [n][S] the keys each row sees; xk [n][E][hd], xv
    [E][hd]: per-row extra keys every row sees (the sinks), E may be 0.  -> (out, bar) [n][hd]."""
    dt = np.float32 if variant == "f32" else np.float64
    q, K, V, xk, xv = (a.astype(dt) for a in (q, K, V, xk, xv))
    E = xv.shape[0]
    sc = dt(scale)
    qs = q_hi(q) if variant == "q_hi_only" else q
    s = np.where(vis, (qs @ K.T) * sc, dt(-np.inf))
    s = np.concatenate([np.einsum("nd,ned->ne", q, xk) * sc, s], axis=1)
    Va = np.concatenate([xv, V], axis=0)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    den = p.sum(axis=1, keepdims=True)
    num = p
    if variant == "p_hi_only":
        num = p.copy()
        num[:, E:] = p[:, E:].astype(np.float32).astype(np.float16).astype(dt)
    out = (num @ Va) / den
    if variant != "f64":
        return out, None
    terms = np.where(vis, np.abs(q) @ np.abs(K).T, 0.0)
    terms = np.concatenate([np.einsum("nd,ned->ne", np.abs(q), np.abs(xk)), terms], axis=1)
    ds = 5e-7 * terms.max(axis=1, keepdims=True) * float(scale)
    return out, (2 * ds + 4e-6) * ((p / den) @ np.abs(Va)) + 1e-7


def _heads(q, K, V, vis, xk, xv, n_heads, n_kv, hd, variant):
    n = q.shape[0]
    qpk = n_heads // n_kv
    q3 = q.reshape(n, n_heads, hd)
    K3, V3 = K.reshape(-1, n_kv, hd), V.reshape(-1, n_kv, hd)
    xk4, xv3 = xk.reshape(n, -1, n_kv, hd), xv.reshape(-1, n_kv, hd)
    out = np.empty((n, n_heads, hd))
    bar = np.empty((n, n_heads, hd)) if variant == "f64" else None
    for h in range(n_heads):
        g = h // qpk
        o, b = _head(q3[:, h], K3[:, g], V3[:, g], vis, xk4[:, :, g], xv3[:, g], attn_scale(hd), variant)
        out[:, h] = o
        if bar is not None:
            bar[:, h] = b
    return out.reshape(n, -1), None if bar is None else bar.reshape(n, -1)


def causal(q, k16, v16, pos0, n_heads, n_kv, hd, variant="f64"):
    """q f32 [n][n_heads hd]; k16, v16 f16 bits [pos0 + n][n_kv hd] -> (out, bar) float64 [n][n_heads hd]
    (bar None unless variant is "f64")."""
    n, S = q.shape[0], k16.shape[0]
    vis = np.arange(S)[None, :] <= pos0 + np.arange(n)[:, None]
    none_k, none_v = np.zeros((n, 0, n_kv * hd)), np.zeros((0, n_kv * hd))
    return _heads(q.astype(np.float64), f16_vals(k16), f16_vals(v16), vis, none_k, none_v, n_heads, n_kv, hd, variant)


def ring_slots(p0, L, count):
    """ring slot of virtual row u = 0 .. count - 1 (count <= W)"""
    W = L - 2
    return 2 + ((p0 - 2) % W + np.arange(count)) % W


def ring(q, k_ring, v_ring, ks, vs, sink_ver, p0, n_heads, n_kv, variant="f64"):
    """The ring pass at head_dim 128: q f32 [m][n_heads 128]; k_ring, v_ring f16 bits [L][kv_dim];
    ks, vs [m][kv_dim]; sink_ver [m][2][kv_dim] -> (out, bar) float64 [m][n_heads 128]."""
    m, L = q.shape[0], k_ring.shape[0]
    W = L - 2
    order = ring_slots(p0, L, W)
    K = np.concatenate([f16_vals(k_ring)[order], f16_vals(ks)], axis=0)  # the virtual key sequence
    V = np.concatenate([f16_vals(v_ring)[order], f16_vals(vs)], axis=0)
    u, t = np.arange(W + m)[None, :], np.arange(m)[:, None]
    vis = (u >= t + 1) & (u <= W + t)
    return _heads(q.astype(np.float64), K, V, vis, f16_vals(sink_ver), f16_vals(v_ring)[:2], n_heads, n_kv, 128, variant)


def ring_after_commit(k_ring, v_ring, ks, vs, sink_ver, p0):
    """The ring as the pass leaves it: exact moves."""
    m, L = ks.shape[0], k_ring.shape[0]
    k2, v2 = k_ring.copy(), v_ring.copy()
    slots = ring_slots(p0, L, m)
    k2[slots], v2[slots] = ks, vs
    k2[:2] = sink_ver[m - 1]
    return k2, v2


# ------------------------------------------------------------------------------------------
# seeded inputs
# ------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=4)
def causal_inputs(n_heads, n_kv, hd, n, pos0, kind="rand"):
    """(q f32, k f16 bits, v f16 bits): q ~ 0.5 N(0, 1), K / V ~ N(0, 1) rounded to f16.  kind "peaked":
    every q row of KV head g also carries 45 u_g (u_g a unit vector), so the other keys score with
    a deviation of 4; K row pos0 + 3 is 8 u_g, a score of 32, and K row 5 is 8 a_g with a_g a unit
    vector at cosine 0.75 to u_g, a score of 24.  Rows t < 3 see the first peak only (weight 1 - 1e-5,
    in the first history split); for the others the max moves to the second peak on the pass's own
    rows, at the end of the walk, and everything before it is rescaled by e^-8 or less.  (Peaks that
    share the mass with other keys fail the bar's own f32 condition: a sequential f32 sum of 128
    products of one sign is off by about the 5e-7 of ds; 24 u_g gave 0.3 of the bar, 45 u_g gives
    0.15, tests/test_prompt_attn_cpu.py.)"""
    rng = _rng("causal", n_heads, n_kv, hd, n, pos0, kind)
    q = (Q_SCALE * rng.standard_normal((n, n_heads * hd))).astype(np.float32)
    k = (KV_STD * rng.standard_normal((pos0 + n, n_kv * hd))).astype(np.float32)
    v = (KV_STD * rng.standard_normal((pos0 + n, n_kv * hd))).astype(np.float32)
    if kind == "peaked":
        u = rng.standard_normal((n_kv, hd))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        r = rng.standard_normal((n_kv, hd))
        r -= (r * u).sum(axis=1, keepdims=True) * u
        a = 0.75 * u + np.sqrt(1 - 0.75 ** 2) * r / np.linalg.norm(r, axis=1, keepdims=True)
        q = (q.reshape(n, n_kv, n_heads // n_kv, hd) + 45.0 * u[None, :, None, :]).reshape(n, -1).astype(np.float32)
        k[5] = (8.0 * a).reshape(-1)
        k[pos0 + 3] = (8.0 * u).reshape(-1)
    for a in (q, k, v):
        a.setflags(write=False)
    kb, vb = f16_bits(k), f16_bits(v)
    kb.setflags(write=False)
    vb.setflags(write=False)
    return q, kb, vb


@functools.lru_cache(maxsize=4)
def ring_inputs(n_heads, n_kv, L, p0, m):
    """(q f32 [m], k_ring, v_ring [L], ks, vs [m], sink_ver [m][2]) f16 bits, all ~ N(0, 1), q ~ 0.5 N(0, 1)"""
    rng = _rng("ring", n_heads, n_kv, L, p0, m)
    kv = n_kv * 128
    q = (Q_SCALE * rng.standard_normal((m, n_heads * 128))).astype(np.float32)
    out = [q] + [f16_bits(KV_STD * rng.standard_normal(s)) for s in ((L, kv), (L, kv), (m, kv), (m, kv), (m, 2, kv))]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


# ------------------------------------------------------------------------------------------
# the case table (the GPU tests run it; test_prompt_attn_cpu.py checks the bar's conditions on it)
# ------------------------------------------------------------------------------------------
Causal = namedtuple("Causal", "group n_heads n_kv hd n pos0 mode nsplit kind")
Ring = namedtuple("Ring", "group n_heads n_kv L p0 m nsplit")

HEAD_SHAPES = [(8, 2, 128), (16, 2, 128), (8, 8, 128), (8, 4, 128), (16, 2, 64), (8, 8, 64), (4, 2, 16)]
SPLIT_SHAPES = [(8, 2, 128), (8, 8, 128)]

CAUSAL_CASES = []
for _mode in (1, 2):
    for _n, _p in ((37, 0), (70, 45)):
        CAUSAL_CASES += [Causal("heads", *_s, _n, _p, _mode, 0, "rand") for _s in HEAD_SHAPES]
CAUSAL_CASES += [Causal("edges", 8, 2, 128, _n, _p, 1, 0, "rand")
                 for _p in (0, 31, 32, 63, 64, 127) for _n in (1, 2, 33, 129, 257)]
CAUSAL_CASES += [Causal("edges", 8, 2, 128, 300, 100, 1, 0, "rand")]  # an odd number of query tiles in the zig-zag
for _s in SPLIT_SHAPES:
    for _n in (5, 40):
        CAUSAL_CASES += [Causal("splits", *_s, _n, 2400, 1, _k, "rand") for _k in (1, 2, 3, 8, 9, 0)]
        CAUSAL_CASES += [Causal("splits", *_s, _n, 700, 1, 2, "rand")]
    CAUSAL_CASES += [Causal("peaked", *_s, 40, 2400, 1, _k, "peaked") for _k in (3, 1)]

RING_CASES = [Ring("ring", *_s[:2], _L, _p0, _m, 1)
              for _s in SPLIT_SHAPES for _L in (66, 130) for _p0 in (_L, _L + 5, 3 * _L + 17) for _m in (3, 33, _L - 2)]
RING_CASES += [Ring("ring-splits", 8, 8, 2306, 2306 + 1000, _m, _k) for _m in (40, 200) for _k in (2, 9, 0)]


def case_id(c):
    if isinstance(c, Causal):
        return f"{c.group}-h{c.n_heads}kv{c.n_kv}d{c.hd}-n{c.n}-pos{c.pos0}-mode{c.mode}-ns{c.nsplit}"
    return f"{c.group}-h{c.n_heads}kv{c.n_kv}-L{c.L}-p{c.p0}-m{c.m}-ns{c.nsplit}"


def inputs(c):
    if isinstance(c, Causal):
        return causal_inputs(c.n_heads, c.n_kv, c.hd, c.n, c.pos0, c.kind)
    return ring_inputs(c.n_heads, c.n_kv, c.L, c.p0, c.m)


def input_key(c):
    """cases that differ in mode / nsplit only share inputs and reference"""
    return c._replace(group="", mode=0, nsplit=0) if isinstance(c, Causal) else c._replace(group="", nsplit=0)


@functools.lru_cache(maxsize=None)
def _evaluate(key, variant):
    if isinstance(key, Causal):
        q, k, v = inputs(key)
        out, bar = causal(q, k, v, key.pos0, key.n_heads, key.n_kv, key.hd, variant)
    else:
        q, kr, vr, ks, vs, sv = inputs(key)
        out, bar = ring(q, kr, vr, ks, vs, sv, key.p0, key.n_heads, key.n_kv, variant)
    for a in (out, bar):
        if a is not None:
            a.setflags(write=False)
    return out, bar


def reference(c):
    """(out, bar) float64 of the case, computed once per distinct input and read-only"""
    return _evaluate(input_key(c), "f64")


def variant(c, name):
    return _evaluate(input_key(c), name)[0]


def fewest_keys(c):
    """the fewest walked keys any row of the case sees (the ring's two sinks aside)"""
    return c.pos0 + 1 if isinstance(c, Causal) else c.L - 2


def ratio(got, c):
    """worst |got - ref| / bar over every row, head and element"""
    ref, bar = reference(c)
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) / bar).max())
