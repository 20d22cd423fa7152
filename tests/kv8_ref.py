"""Reference forward for an fp8 (e4m3) KV ring, built from the CPU oracle's own ops.

One step is composed layer by layer from O.rmsnorm, O.matmul, O.rope and O.mha, as
tests/stage_ref.py's oracle_observe composes one.  The K/V rows are kept as e4m3 codes and handed
to O.mha as their fp16 image: every e4m3 value is exact in fp16 (test_kv8_cpu checks all 254
finite codes), so O.mha is a valid reference unchanged.  The two sink rows of K live in an fp16
master per layer: past the ring wrap the master rotates (the oracle's rope at pos = 1, rounded to
fp16) and ring slot r is rewritten as f8(master[r]).

Verify, then adopt.  A matvec that differs from the oracle's in the last f32 bits can land on the
other side of an e4m3 rounding boundary, and one such element would send the two forwards apart
for the rest of the sequence.  So for every element the device wrote in the step (read back with
kv_read8, kv_sink_read for the master) the reference checks

    |image(code) - k_ref| <= ulp8(k_ref) / 2 + eps

with k_ref its own unrounded f32 value (clamped to +-448, as the definition clamps), ulp8 the e4m3
spacing at k_ref (2^-9 in the subnormal range) and eps the qkv stage's f32 bar of
tests/stage_ref.py: 2e-6 sum|w||x| + 1e-7 through the 1-Lipschitz clip, then the rotated bars plus
4e-6 max(|v0|, |v1|) for the RoPE pair.  No element is exempt.  Then it continues from the device's
code.  The master's rows are fp16: their bar is stage_ref's f16-row bar (the f32 bar of the rotation,
4e-6 max(|v0|, |v1|), plus one f16 ulp |ref| 2^-10 + 2^-24), and the ring's sink slots must equal
f8(master) of the adopted master bit for bit.
"""
import numpy as np

from oracle import oracle as O
from xalm_amd import _lib as L

import stage_ref as SR

# ---- e4m3fn: the 256 codes' values (NaN at 0x7F / 0xFF) ------------------------------------------
_c = np.arange(256)
_e, _m = (_c >> 3) & 15, _c & 7
VALUES = np.where(_e > 0, (8 + _m) * 2.0 ** (_e - 10.0), _m * 2.0 ** -9)
VALUES = np.where(_c & 0x80, -VALUES, VALUES).astype(np.float64)
VALUES[[0x7F, 0xFF]] = np.nan
FINITE = np.array([c for c in range(256) if c not in (0x7F, 0xFF)], dtype=np.uint8)
IMAGE_F16 = np.nan_to_num(VALUES).astype(np.float16)  # exact for every finite code


def image16(codes):
    """e4m3 codes -> the fp16 bits of their values (what O.mha reads)."""
    return IMAGE_F16[np.asarray(codes, np.uint8)].view(np.uint16)


def image64(codes):
    return VALUES[np.asarray(codes, np.uint8)]


def quantize_search(v):
    """The nearest finite e4m3 value of each v (after the +-448 clamp) by float64 search, ties to
    the even code; the sign of v kept on a zero result.  The independent check of the host definition."""
    v = np.asarray(v, np.float64)
    mag = np.minimum(np.abs(v), 448.0)
    pos = VALUES[:0x7F]  # codes 0 .. 0x7E, ascending
    d = np.abs(mag[..., None] - pos)
    best = d.min(axis=-1, keepdims=True)
    cand = d == best  # one code, or the two neighbours of a midpoint
    even = cand & ((np.arange(0x7F) & 1) == 0)
    pick = np.where(cand.sum(axis=-1) > 1, even.argmax(axis=-1), cand.argmax(axis=-1))
    return (pick | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8)


def ulp8(v):
    """e4m3 spacing at |v| (2^-9 below the least normal 2^-6; the top binade's above 256)."""
    a = np.minimum(np.abs(np.asarray(v, np.float64)), 448.0)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -6)))
    return 2.0 ** (e - 3)


def quantizer_inputs():
    """Every finite f16 value; every midpoint of adjacent e4m3 values with its f32 neighbours on
    both sides; the clamp's edges; signed zeros; 2^-10 (the tie that gives zero) and its neighbours."""
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    f16 = h[np.isfinite(h)].astype(np.float32)
    pos = VALUES[:0x7F]
    mid = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)  # exact in f32
    mids = np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))])
    t = np.float32(2.0 ** -10)
    edge = np.array([448, 449, 1e9, 0.0, t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))], np.float32)
    x = np.concatenate([f16, mids, -mids, edge, -edge]).astype(np.float32)
    assert np.isfinite(x).all()
    return x


class Kv8Ref:
    def __init__(self, xf, context=0):
        c = self.c = xf.config(context)
        self.q_dim, self.kv_dim = c.n_heads * c.head_dim, c.n_kv_heads * c.head_dim
        rows = {L.EMBED: c.vocab_size, L.WCLS: c.vocab_size, L.WQ: self.q_dim, L.WK: self.kv_dim, L.WV: self.kv_dim,
                L.WO: c.dim, L.W1: c.hidden_dim, L.W3: c.hidden_dim, L.W2: c.dim}
        load = lambda k, n: (xf.dtype(n), np.ascontiguousarray(xf.raw(n)).reshape(rows.get(k, 1), -1))  # [rows][row bytes]
        self.glob = {k: load(k, n) for k, n in xf.global_tensors(bool(c.tie_word_embeddings)).items()}
        self.lay = [{k: load(k, n) for k, n in xf.layer_tensors(l).items()} for l in range(c.n_layers)]
        # |w| of Wk / Wv in float64, for the qkv stage's bar
        self.mag = [{k: SR.decode64(*w[k], c.dim)[1] for k in (L.WK, L.WV)} for w in self.lay]
        self.reset()
        self.worst = 0.0  # the largest err / bound any verified element reached

    def reset(self):
        c = self.c
        self.k = np.zeros((c.n_layers, c.max_seq_len, self.kv_dim), np.uint8)
        self.v = np.zeros_like(self.k)
        self.master = np.zeros((c.n_layers, 2, self.kv_dim), np.uint16)

    def _mm(self, x, w, n, d):
        dt, raw = w
        if dt in (L.Q4_1, L.Q5_0, L.Q5_1):
            return O.matmul(x, SR.decode64(dt, raw, n)[0].astype(np.float32), L.F32, n, d)
        return O.matmul(x, raw, dt, n, d)

    def _rope_cs(self, pos):
        c = self.c
        val = np.zeros(c.head_dim // 2, np.float32)
        for j in range(0, c.head_dim, 2):
            if j < c.rotary_dim:
                freq = np.float32(1.0) / np.float32(SR._libm.powf(np.float32(c.rope_theta), np.float32(j) / np.float32(c.rotary_dim)))
                val[j // 2] = np.float32(pos) * freq
        return np.cos(val.astype(np.float64)), np.sin(val.astype(np.float64))

    def _verify(self, what, codes, ref, eps):
        ref = np.clip(np.asarray(ref, np.float64), -448.0, 448.0)
        err = np.abs(image64(codes) - ref)
        bound = ulp8(ref) / 2 + eps
        bad = np.flatnonzero(~(err <= bound))
        assert bad.size == 0, (what, int(bad[0]), float(err[bad[0]]), float(bound[bad[0]]), int(codes[bad[0]]), float(ref[bad[0]]))
        self.worst = max(self.worst, float((err / bound).max()))

    def step(self, token, pos, gm):
        """One token at `pos`, after the device (gm, an fp8-KV Model) ran the same token: verifies
        and adopts the device's K/V codes (and past the wrap its sink master) of every layer, and
        returns the reference logits."""
        c, f32 = self.c, np.float32
        msl = c.max_seq_len
        sink = 2 if pos >= msl else 0
        kv_pos = sink + (pos - sink) % (msl - sink)
        kv_len = min(pos + 1, msl)
        head = type("H", (), {"head_dim": c.head_dim})
        cs = self._rope_cs(pos)
        clipv = lambda a: np.clip(a, -f32(c.qkv_clip), f32(c.qkv_clip)).astype(f32)
        edt, emb = self.glob[L.EMBED]
        x = SR.decode64(edt, emb[token:token + 1], c.dim)[0][0].astype(f32)
        for l, w in enumerate(self.lay):
            ndt, nw = w[L.ATTN_NORM]
            xn = O.rmsnorm(x, nw.reshape(-1), ndt, c.norm_eps)
            q = O.rope(clipv(self._mm(xn, w[L.WQ], c.dim, self.q_dim)), c.head_dim, pos, c.rope_theta, c.rotary_dim)
            kc = clipv(self._mm(xn, w[L.WK], c.dim, self.kv_dim))
            k = O.rope(kc, c.head_dim, pos, c.rope_theta, c.rotary_dim)
            v = clipv(self._mm(xn, w[L.WV], c.dim, self.kv_dim))
            ax = np.abs(xn.astype(np.float64))
            bk = SR.rope_bar(head, kc.astype(np.float64), 2e-6 * (self.mag[l][L.WK] @ ax) + 1e-7, cs)[1]
            bv = 2e-6 * (self.mag[l][L.WV] @ ax) + 1e-7
            if sink:
                # the sinks rotate in the master (rope at pos = 1, rounded to fp16); the ring's rows follow
                dev_m = gm.kv_sink_read(l)
                dev_ring = gm.kv_read8(l, 0, 0, 2)
                for r in range(2):
                    old = self.master[l, r].view(np.float16).astype(f32)
                    new = O.rope(old, c.head_dim, 1, c.rope_theta, c.rotary_dim).astype(np.float64)
                    pair = np.maximum(np.abs(old[0::2]), np.abs(old[1::2])).astype(np.float64).repeat(2)
                    bound = 4e-6 * pair + np.abs(new) * 2.0 ** -10 + 2.0 ** -24
                    err = np.abs(dev_m[r].view(np.float16).astype(np.float64) - new)
                    assert (err <= bound).all(), ("master", l, r, pos, float((err / bound).max()))
                    self.worst = max(self.worst, float((err / bound).max()))
                self.master[l] = dev_m
                want = L.f8_e4m3_from_f32(dev_m.view(np.float16).astype(f32))
                assert np.array_equal(dev_ring, want), ("ring sink != f8(master)", l, pos)
                self.k[l, 0:2] = dev_ring
            dk, dv = gm.kv_read8(l, 0, kv_pos, 1)[0], gm.kv_read8(l, 1, kv_pos, 1)[0]
            self._verify(("k", l, pos), dk, k, bk)
            self._verify(("v", l, pos), dv, v, bv)
            self.k[l, kv_pos], self.v[l, kv_pos] = dk, dv
            if kv_pos < 2:  # the master starts as the exact image of the first two K rows
                self.master[l, kv_pos] = image16(dk)
                assert np.array_equal(gm.kv_sink_read(l)[kv_pos], self.master[l, kv_pos]), ("master image", l, pos)
            att = O.mha(image16(self.k[l]), image16(self.v[l]), q, c.head_dim, kv_len, msl, c.n_heads, c.n_kv_heads)
            x = (x + self._mm(att, w[L.WO], self.q_dim, c.dim)).astype(f32)
            ndt, nw = w[L.FFN_NORM]
            xn1 = O.rmsnorm(x, nw.reshape(-1), ndt, c.norm_eps)
            g, u = self._mm(xn1, w[L.W1], c.dim, c.hidden_dim), self._mm(xn1, w[L.W3], c.dim, c.hidden_dim)
            if c.act == L.ACT_SILU:
                a = (g / (f32(1) + np.exp(-g, dtype=f32))).astype(f32)
            else:
                a = (f32(0.5) * g * (f32(1) + np.tanh(f32(0.797885) * (g + f32(0.044715) * g * g * g), dtype=f32))).astype(f32)
            x = (x + self._mm((a * u).astype(f32), w[L.W2], c.hidden_dim, c.dim)).astype(f32)
        ndt, nw = self.glob[L.FINAL_NORM]
        xn = O.rmsnorm(x, nw.reshape(-1), ndt, c.norm_eps)
        wc = self.glob[L.EMBED] if c.tie_word_embeddings else self.glob[L.WCLS]
        return self._mm(xn, wc, c.dim, c.vocab_size)
