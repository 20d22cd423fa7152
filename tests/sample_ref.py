"""Reference for the seeded sampler (xh_sampling, include/xalm_hip.h) in numpy float64, with its own
restatement of Philox4x32-10, and the case lists the CPU and GPU tests share.

For one (logits, temperature, top_k, top_p) it gives the kept set and the band: the tokens whose
membership in the nucleus lies within DELTA of the cut, |prefix mass before the token - top_p W_S|
< DELTA W_S, with W_S the top-k set's mass.  The first token in the order is never in the band: it
is kept whatever the cut ("at least one token is always kept").  A case with a non-empty band is
undecided and is skipped by the tests (at most SKIP_CAP of the generated cases of a test; none of
the named edge cases).  For a draw it gives the accepted tokens: kept tokens of non-zero weight
whose interval [cum_before - DELTA W, cum_after + DELTA W) in ascending index order contains u W.

DELTA = 2e-5: a fixed-order f32 sum of V <= 128256 positive terms (about 125 sequential adds per
thread plus a 10-level tree) is off by at most about 135 * 2^-24 = 8e-6 relative, expf adds a few
1e-7; DELTA is twice that worst case.  The device's integer masses (w * 2^40 truncated) are off by
less than V * 2^-40 = 1.2e-7 of the total.

Choices the definition leaves open, as the device and the host mirror make them: with no finite
logit the token is 0 and n_kept is 0; greedy (temperature 0) reports n_kept 1; the counter's first
word is pos mod 2^32.
"""
from functools import lru_cache

import numpy as np

DELTA = 2e-5
SKIP_CAP = 0.10
FLT_MIN = float(np.finfo(np.float32).tiny)
M32 = 0xFFFFFFFF


def philox4x32(seed: int, pos: int):
    """Philox4x32-10: key (seed & 0xffffffff, seed >> 32), counter (pos mod 2^32, 0, 0, 0)."""
    k0, k1 = seed & M32, (seed >> 32) & M32
    c = [pos & M32, 0, 0, 0]
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c


def uniform(seed: int, pos: int) -> float:
    return (philox4x32(seed, pos)[0] >> 8) * 2.0 ** -24


def order_keys(logits: np.ndarray) -> np.ndarray:
    """uint32 keys: a larger logit (by its f32 bits) has a larger key."""
    u = np.ascontiguousarray(logits, dtype=np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


class Analysis:
    """kept: token ids of the kept set (ascending); n_kept; band: token ids (empty = decided);
    w: float64 weights [V]."""

    def __init__(self, logits, temperature, top_k, top_p):
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        V = lg.size
        self.V = V
        self.greedy = float(np.float32(temperature)) == 0.0
        self.band = np.zeros(0, dtype=np.int64)
        self.w = None
        if self.greedy:
            ok = lg > np.float32(FLT_MIN)
            tok = int(np.argmax(np.where(ok, lg, -np.inf))) if ok.any() else 0
            self.kept = np.array([tok])
            self.n_kept = 1
            return
        m = float(lg.max())
        if not np.isfinite(m):
            self.kept = np.zeros(0, dtype=np.int64)
            self.n_kept = 0
            return
        T = float(np.float32(temperature))
        P = float(np.float32(top_p))
        with np.errstate(over="ignore", invalid="ignore"):
            w = np.exp((lg.astype(np.float64) - m) / T)
        w[np.isneginf(lg)] = 0.0
        self.w = w
        order = np.lexsort((np.arange(V), M32 - order_keys(lg).astype(np.int64)))
        n_k = min(top_k, V) if top_k > 0 else V
        order = order[:n_k]
        if P < 1.0:
            ws = w[order]
            W_S = ws.sum()
            before = np.cumsum(ws) - ws
            inside = before < P * W_S
            inside[0] = True
            near = np.abs(before - P * W_S) < DELTA * W_S
            near[0] = False
            self.band = order[near]
            order = order[inside]
        self.kept = np.sort(order)
        self.n_kept = int(self.kept.size)

    @property
    def decided(self):
        return self.band.size == 0

    def accepted(self, seed: int, pos: int):
        """Token ids a correct sampler may return for the draw at counter pos."""
        if self.greedy:
            return {int(self.kept[0])}
        if self.n_kept == 0:
            return {0}
        wk = self.w[self.kept]
        W = wk.sum()
        after = np.cumsum(wk)
        before = after - wk
        x = uniform(seed, pos) * W
        ok = (before - DELTA * W <= x) & (x < after + DELTA * W) & (wk > 0)
        return set(int(t) for t in self.kept[ok])


# ---- the case lists -------------------------------------------------------------------------
SEED = 0x5EED0123456789AB  # both key words non-zero
N_DRAWS = 64
POS0 = 17
VOCABS = (300, 32000, 128256)


@lru_cache(maxsize=None)
def peaked_logits(V: int) -> np.ndarray:
    """8 * N(0, 1): peaked like a language model's."""
    lg = (8.0 * np.random.default_rng(1000 + V).standard_normal(V)).astype(np.float32)
    lg.setflags(write=False)
    return lg


def grid(V: int):
    """(temperature, top_k, top_p) of the op test at vocabulary V."""
    return [(t, k, p) for t in (0.7, 1.5) for k in (0, 1, 40, V, V + 5) for p in (1.0, 0.9, 1e-6)]


@lru_cache(maxsize=None)
def grid_analysis(V: int, t: float, k: int, p: float) -> Analysis:
    return Analysis(peaked_logits(V), t, k, p)


def edge_cases():
    """name -> (logits, temperature, top_k, top_p, expected kept ids or None): every one must be decided."""
    rng = np.random.default_rng(7)
    V = 300
    out = {}
    out["all_equal_top3"] = (np.full(V, 1.25, np.float32), 1.0, 3, 1.0, [0, 1, 2])
    lg = rng.standard_normal(V).astype(np.float32)
    lg[[7, 120]] = 9.0
    lg[[10, 50, 51, 200]] = 5.0  # places 3..6: top_k 4 takes 10 and 50
    out["tie_at_kth"] = (lg, 1.0, 4, 1.0, [7, 10, 50, 120])
    lg = (8.0 * rng.standard_normal(V)).astype(np.float32)
    lg[64:192] = -np.inf
    out["neg_inf_block"] = (lg, 1.5, 0, 1.0, list(range(V)))
    out["neg_inf_block_top_p"] = (lg.copy(), 1.5, 0, 0.9, None)
    out["neg_inf_block_top_k"] = (lg.copy(), 1.5, 200, 1.0, None)
    out["all_neg_inf"] = (np.full(V, -np.inf, np.float32), 1.0, 0, 1.0, [])
    out["magnitude_1e4"] = ((1e4 * rng.standard_normal(V)).astype(np.float32), 0.7, 40, 0.9, None)
    lg = rng.standard_normal(V).astype(np.float32)
    lg[[33, 210]] = 6.5  # the maximum twice: the first one is kept
    out["top_p_tiny"] = (lg, 1.0, 0, 1e-6, [33])
    lg = -np.abs(rng.standard_normal(V)).astype(np.float32)
    lg[5] = np.float32(FLT_MIN)
    out["greedy_all_tiny"] = (lg, 0.0, 5, 0.5, [0])
    for v in out.values():
        v[0].setflags(write=False)
    return out
