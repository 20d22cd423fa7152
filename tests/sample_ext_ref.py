"""Reference for the extended draw (xh_logit_ctl, include/xalm_hip.h), on top of sample_ref: the
adjustment l' in numpy float32 with every operation rounded separately, the min-p prefix and the
log-probability in float64, and the case lists the CPU and GPU tests share.

Min-p adds a band to sample_ref's: a case is undecided when any token's float64 weight lies within
DELTA * min_p of min_p.  The maxima of l' are never in that band: their weight is exp(0) = 1 in any
arithmetic and min_p <= 1, so they are kept whatever the rounding (as the first token of the order
is never in the top-p band).

Log-probability bound: |lp - lp64| <= 2e-5 + 2^-21 * max(1, |lp64|).  2e-5 is sample_ref's DELTA, the
bound on an f32 sum of V positive terms, taken as an absolute error of its log; the subtraction, logf
and the final subtraction contribute at most about 2^-24 relative each, and the bound doubles the sum
of those.
"""
from collections import Counter
from functools import lru_cache

import numpy as np

import sample_ref as R

F = np.float32
NEG_INF = float("-inf")


def adjust(logits, window=(), repeat_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, last_n=0, min_p=0.0,
           logit_bias=None):
    """l' [V] float32: one float32 operation per step of the definition.  min_p is accepted and
    ignored, so a controls dict can be passed whole."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    out = lg.copy()
    win = list(window)
    n = min(int(last_n), len(win))
    counts = Counter(int(t) for t in win[len(win) - n:]) if n else Counter()
    bias = dict(logit_bias.items() if isinstance(logit_bias, dict) else (logit_bias or ()))
    rp, pp, fp = F(repeat_penalty), F(presence_penalty), F(frequency_penalty)
    with np.errstate(all="ignore"):
        for t in set(counts) | set(bias):
            a = lg[t]
            if t in bias:
                a = F(a + F(bias[t]))
            c = counts.get(t, 0)
            if c > 0:
                r = F(a / rp) if a > 0 else F(a * rp)
                r = F(r - F(F(c) * fp))
                a = F(r - pp)
            out[t] = a
    return out


class ExtAnalysis(R.Analysis):
    """sample_ref.Analysis of l' under the effective top-k min(top_k or V, n_minp)."""

    def __init__(self, adjusted, temperature, top_k, top_p, min_p):
        lg = np.ascontiguousarray(adjusted, dtype=np.float32)
        T, mp = float(F(temperature)), float(F(min_p))
        self.minp_band = np.zeros(0, dtype=np.int64)
        self.n_minp = None
        k = top_k
        m = float(lg.max())
        if T > 0.0 and mp > 0.0 and np.isfinite(m):
            with np.errstate(over="ignore", invalid="ignore"):
                w = np.exp((lg.astype(np.float64) - m) / T)
            w[np.isneginf(lg)] = 0.0
            self.n_minp = int((w >= mp).sum())
            self.minp_band = np.flatnonzero((np.abs(w - mp) < R.DELTA * mp) & (lg != F(m)))
            k = min(top_k, self.n_minp) if top_k > 0 else self.n_minp
        super().__init__(lg, temperature, k, top_p)

    @property
    def decided(self):
        return self.band.size == 0 and self.minp_band.size == 0


def logprob64(logits, tok):
    lg = np.ascontiguousarray(logits, dtype=np.float32).astype(np.float64)
    m = lg.max()
    return float((lg[tok] - m) - np.log(np.exp(lg - m).sum()))


def logprob_bound(lp64):
    return 2e-5 + 2.0 ** -21 * max(1.0, abs(lp64))


def parity_bound(logits):
    """The project's logit parity bound (the forward tests'): 1e-3 * max(1, max |logit|)."""
    return 1e-3 * max(1.0, float(np.abs(logits).max()))


# ---- the adjustment's case list (CPU: xh_adjust_logits; GPU: adjusted_out of xh_op_sample_ext) ------
ADJ_VOCABS = (300, 128256)
ALL3 = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2)
# 7 sits in the window, 11 and 12 outside it, 8 in the window and banned
BIAS = [(7, 1.5), (11, -2.25), (12, NEG_INF), (8, NEG_INF)]


@lru_cache(maxsize=None)
def adjust_logits_vector(V):
    lg = R.peaked_logits(V).copy()
    lg[5] = -0.0
    lg[6] = -np.inf
    lg[7] = abs(lg[7]) + 1.0   # a positive and a negative logit under the repeat penalty
    lg[9] = -abs(lg[9]) - 1.0
    lg[0] = 3.25
    lg[V - 1] = -4.5
    lg.setflags(write=False)
    return lg


@lru_cache(maxsize=None)
def adjust_cases(V):
    """name -> (window, controls): windows of 0, 1, 64 and 1024 tokens, a token three times, tokens
    0 and V-1, -0.0 (5) and -inf (6) raw logits, biases inside and outside the window, a -inf bias,
    both signs under repeat 1.3 and 0.8, each penalty alone and all three."""
    rng = np.random.default_rng(4000 + V)
    w64 = [0, V - 1, 5, 6, 7, 8, 9, 9, 9] + rng.integers(16, V, 55).tolist()
    assert len(w64) == 64
    w1024 = rng.integers(16, min(V, 400), 1024 - 9).tolist() + [0, V - 1, 5, 6, 7, 8, 9, 9, 9]
    out = {
        "window_0": ([], dict(ALL3, last_n=64, logit_bias=BIAS)),
        "window_1": ([9], dict(ALL3, last_n=1)),
        "repeat_1.3": (w64, dict(repeat_penalty=1.3, last_n=64)),
        "repeat_0.8": (w64, dict(repeat_penalty=0.8, last_n=64)),
        "presence": (w64, dict(presence_penalty=0.5, last_n=64)),
        "frequency": (w64, dict(frequency_penalty=0.2, last_n=64)),
        "all_three": (w64, dict(ALL3, last_n=64)),
        "all_three_bias": (w64, dict(ALL3, last_n=64, logit_bias=BIAS)),
        "negative_penalties": (w64, dict(repeat_penalty=0.8, presence_penalty=-0.3, frequency_penalty=-0.1, last_n=64,
                                         logit_bias=BIAS)),
        "window_1024": (w1024, dict(ALL3, last_n=1024, logit_bias=BIAS)),
        "tail_of_longer": (w1024[:36] + w64, dict(ALL3, last_n=64, logit_bias=BIAS)),  # only the last 64 count
        "last_n_0": (w64, dict(ALL3, last_n=0, logit_bias=BIAS)),                   # penalties off, biases on
        "bias_256": (w64, dict(ALL3, last_n=64, logit_bias=[(t, -1.0 - 0.01 * t) for t in range(256)])),
    }
    return out


# ---- the draws' case list --------------------------------------------------------------------------
CTL_ON = dict(ALL3, last_n=64)


@lru_cache(maxsize=None)
def draw_window(V):
    """64 tokens with duplicates, the eight largest logits three times each among them."""
    lg = R.peaked_logits(V)
    top = np.argsort(lg)[-8:].tolist()
    rest = np.random.default_rng(5000 + V).integers(0, V, 40).tolist()
    return tuple(top * 3 + rest)


def draw_grid():
    """(temperature, top_k, top_p, min_p, controls on) of the draw test."""
    return [(t, k, p, mp, on) for t in (0.7, 1.5) for k in (0, 40) for p in (1.0, 0.9) for mp in (0.0, 0.05, 1.0)
            for on in (False, True)]


@lru_cache(maxsize=None)
def draw_adjusted(V, on):
    out = adjust(R.peaked_logits(V), draw_window(V), **CTL_ON) if on else R.peaked_logits(V).copy()
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def draw_analysis(V, t, k, p, mp, on):
    return ExtAnalysis(draw_adjusted(V, on), t, k, p, mp)


def edge_cases():
    """name -> (logits, window, temperature, top_k, top_p, controls, expected kept ids or None):
    every one must be decided."""
    V = 300
    rng = np.random.default_rng(11)
    out = {}
    lg = rng.standard_normal(V).astype(np.float32)
    lg[40], lg[41] = 9.0, 8.5  # the raw argmax is demoted below the runner-up: 9 / 2 - 0 - 0 = 4.5
    out["greedy_demoted"] = (lg, [40, 3, 3], 0.0, 0, 1.0, dict(repeat_penalty=2.0, last_n=3), [41])
    out["ban_argmax"] = (lg.copy(), [], 1.0, 0, 1.0, dict(logit_bias=[(40, NEG_INF)]), None)
    lg2 = rng.standard_normal(V).astype(np.float32)
    lg2[[17, 99, 250]] = 6.0   # min_p 1 keeps exactly the maxima
    out["min_p_1_maxima"] = (lg2, [], 0.7, 0, 1.0, dict(min_p=1.0), [17, 99, 250])
    # ... of l', not of l: 17 is in the window, so 99 and 250 remain
    out["min_p_1_adjusted"] = (lg2.copy(), [17], 0.7, 0, 1.0, dict(min_p=1.0, presence_penalty=0.5, last_n=1), [99, 250])
    out["min_p_under_top_k"] = (lg2.copy(), [], 1.0, 2, 1.0, dict(min_p=1.0), [17, 99])
    for v in out.values():
        v[0].setflags(write=False)
    return out


def edge_analysis(name):
    lg, win, t, k, p, ctl, kept = edge_cases()[name]
    return ExtAnalysis(adjust(lg, win, **ctl), t, k, p, ctl.get("min_p", 0.0))
