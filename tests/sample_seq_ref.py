"""Reference for the sequence-aware draw (xh_seq_ctl, include/xalm_hip.h), on top of sample_ref,
sample_ext_ref and sample_adapt_ref: the match lengths by brute force over the window, DRY's penalty
loop in numpy float32 (one rounding per operation), the n-gram ban, XTC on sample_adapt_ref's integer
masses with the coin from sample_ref's Philox, and the case lists the CPU and GPU tests share.

Nothing in DRY or the ban is ever undecided: match lengths are integers and the penalty is a fixed
sequence of f32 operations, so l', rep_c and ng_c are compared bit for bit.

An XTC case is undecided (skipped; at most sample_ref.SKIP_CAP of a grid, none of the named edge
cases) when sample_adapt_ref's analysis of the stages in front of it is, or when some M_i of C lies
within sample_ref.DELTA * S_C of the cut: the device's expf may differ from numpy's by an ulp or two,
2^-22 relative on a mass and on S_C, far inside DELTA.  Equal logits give equal masses in any
arithmetic, so the choice among A's lowest key is exact.  The coin compares two f32 values and is
never undecided.  The survivors' draw is sample_ref's, with its own top-p band.
"""
import math
from functools import lru_cache

import numpy as np

import sample_adapt_ref as A
import sample_ext_ref as X
import sample_ref as R

F = np.float32
NEG_INF = float("-inf")
MAX_MATCH = 64
MAX_WINDOW = 1024
SEQ_OFF = dict(dry_multiplier=0.0, dry_base=1.75, dry_allowed_length=2, no_repeat_ngram=0, seq_last_n=0, breakers=(),
               xtc_probability=0.0, xtc_threshold=0.1)


def match_lengths(w, breakers=()):
    """({c: rep_c}, {c: ng_c}) of the window w, by the definition's words."""
    w = [int(t) for t in w]
    n = len(w)
    brk = set(int(b) for b in breakers)
    rep, ng = {}, {}
    for j in range(n - 1):
        if w[j] != w[n - 1]:
            continue
        raw = 0
        while raw < min(j + 1, MAX_MATCH) and w[j - raw] == w[n - 1 - raw]:
            raw += 1
        dry = 0
        while dry < raw and w[n - 1 - dry] not in brk:
            dry += 1
        c = w[j + 1]
        rep[c] = max(rep.get(c, 0), dry)
        ng[c] = max(ng.get(c, 0), raw)
    return rep, ng


def seq_adjust(adjusted, window=(), dry_multiplier=0.0, dry_base=1.75, dry_allowed_length=2, no_repeat_ngram=0,
               seq_last_n=0, breakers=(), **_xtc):
    """(l' after DRY and the ban float32 [V], rep_c int32 [V], ng_c int32 [V]) from l' after xh_logit_ctl."""
    out = np.ascontiguousarray(adjusted, dtype=F).copy()
    V = out.size
    rep_v, ng_v = np.zeros(V, np.int32), np.zeros(V, np.int32)
    win = list(window)
    n = min(int(seq_last_n), len(win), MAX_WINDOW)
    mult, base = F(dry_multiplier), F(dry_base)
    if (mult > 0 or no_repeat_ngram >= 2) and n >= 2:
        rep, ng = match_lengths(win[len(win) - n:], breakers)
        with np.errstate(all="ignore"):
            for c in ng:
                rep_v[c], ng_v[c] = rep[c], ng[c]
                if mult > 0 and rep[c] >= dry_allowed_length:
                    p = mult
                    for _ in range(rep[c] - dry_allowed_length):
                        p = F(p * base)
                    out[c] = F(out[c] - p)
                if no_repeat_ngram >= 2 and ng[c] >= no_repeat_ngram - 1:
                    out[c] = F(NEG_INF)
    return out, rep_v, ng_v


def coin(seed, pos, probability):
    """Whether XTC fires for the draw at counter pos: Philox word x1, compared in f32."""
    u = (R.philox4x32(seed, pos)[1] >> 8) * 2.0 ** -24   # 24 bits: exact in f32
    return u < float(F(probability))


class SeqAnalysis:
    """The draw on l'' (adjusted, sequence-adjusted and masked) at temperature > 0 with XTC behind
    sample_adapt_ref's stages.  off: the AdaptAnalysis (what a draw whose coin does not fire, or whose
    A has fewer than two tokens, sees); kept_on / final_on / n_kept_on: the set after XTC, the
    sample_ref.Analysis of the survivors and the size the device reports, for a draw whose coin fires;
    n_a: |A|; reasons: why a fired draw is undecided (off.reasons: any draw)."""

    def __init__(self, lpp, temperature, xtc_probability=0.0, xtc_threshold=0.1, top_k=0, top_p=1.0, min_p=0.0,
                 typical_p=1.0, top_n_sigma=0.0):
        lg = np.ascontiguousarray(lpp, dtype=F)
        self.prob = float(F(xtc_probability))
        self.off = A.AdaptAnalysis(lg, temperature, top_k=top_k, top_p=top_p, min_p=min_p, typical_p=typical_p,
                                   top_n_sigma=top_n_sigma)
        self.reasons = []
        self.kept_on, self.final_on, self.n_kept_on, self.n_a = self.off.kept_map, self.off.final, self.off.n_kept, 0
        if not np.isfinite(float(lg.max())) or self.prob == 0.0:
            return
        C = self.off.kept_map.astype(bool)
        M = A.masses(lg, float(F(temperature)))
        S = int(M[C].sum())
        cut = int(math.ceil(float(F(xtc_threshold)) * float(S)))
        if (C & (np.abs(M.astype(np.float64) - cut) <= R.DELTA * S)).any():
            self.reasons.append("XTC cut")
        in_a = C & (M >= cut)
        self.n_a = int(in_a.sum())
        if self.n_a >= 2:
            keys = R.order_keys(lg)
            kmin = keys[in_a].min()
            last = int(np.flatnonzero(in_a & (keys == kmin)).max())
            kept = C & ~in_a
            kept[last] = True
            self.kept_on = kept.astype(np.uint8)
            cutlg = np.where(kept, lg, F(NEG_INF)).astype(F)
            self.final_on = R.Analysis(cutlg, temperature, 0, top_p)
            self.n_kept_on = self.final_on.n_kept if float(F(top_p)) < 1.0 else int(kept.sum())
            if self.final_on.band.size:
                self.reasons.append("top-p band behind XTC")

    def fired(self, seed, pos):
        return self.prob > 0.0 and coin(seed, pos, self.prob)

    def decided(self, fired):
        return not self.off.reasons and not (fired and self.reasons)

    def view(self, fired):
        """(kept map, final Analysis, n_kept) of a draw."""
        if fired and self.n_a >= 2:
            return self.kept_on, self.final_on, self.n_kept_on
        return self.off.kept_map, self.off.final, self.off.n_kept


# ---- the case lists -------------------------------------------------------------------------
VOCABS = (300, 1500, 131072)


@lru_cache(maxsize=None)
def logits(V):
    """sample_ref's peaked logits (its seed leaves at most SKIP_CAP of the XTC grid undecided at every
    vocabulary here: test_sample_seq_cpu.py checks it)."""
    return R.peaked_logits(V)


def xtc_grid():
    """(temperature, top_k, typical_p, top_p, xtc_probability, xtc_threshold) of the op test."""
    return [(t, k, ty, p, pr, th) for t in (0.7, 1.5) for k in (0, 40) for ty in (1.0, 0.9) for p in (1.0, 0.9)
            for pr in (1.0, 0.5) for th in (0.1, 0.02)]


@lru_cache(maxsize=None)
def xtc_analysis(V, t, k, ty, p, pr, th):
    return SeqAnalysis(logits(V), t, xtc_probability=pr, xtc_threshold=th, top_k=k, top_p=p, typical_p=ty)


@lru_cache(maxsize=None)
def grid_window(V, n):
    """n tokens over an alphabet of 12 ids spread over the vocabulary (0 and V - 1 among them), with a
    planted repeat of the last 70 tokens so a match runs into the cap."""
    rng = np.random.default_rng(6000 + V + n)
    alphabet = np.unique(np.concatenate([[0, V - 1], rng.integers(1, V - 1, 10)]))
    w = alphabet[rng.integers(0, alphabet.size, n)].tolist()
    if n >= 300:
        w[n - 220:n - 150] = w[n - 70:]
    return tuple(int(t) for t in w)


def dry_grid():
    """(window length, seq controls) of the adjustment's test: every window length at which the code
    takes another path, DRY alone, the ban alone and both, breakers on and off."""
    out = []
    for n in (0, 1, 2, 3, 64, 65, 1023, 1024, 1100):
        for kw in (dict(dry_multiplier=0.8, dry_base=1.75, dry_allowed_length=2),
                   dict(no_repeat_ngram=3),
                   dict(dry_multiplier=1.25, dry_base=1.1, dry_allowed_length=1, no_repeat_ngram=5, with_breakers=True)):
            for last_n in (1024, 37):
                out.append((n, dict(kw, seq_last_n=last_n)))
    return out


def grid_controls(V, kw):
    kw = dict(kw)
    if kw.pop("with_breakers", False):
        kw["breakers"] = tuple(sorted(set(grid_window(V, 1100)))[::3])
    return kw


BIG = 1e30


def edge_cases():
    """name -> (V, logits, window, seq controls, logit_ctl controls, {token: (rep_c, ng_c)} expected or
    None): the adjustment's named cases.  The logit_ctl controls are applied first
    (sample_ext_ref.adjust), as the definition orders the stages."""
    out = {}
    rng = np.random.default_rng(31)
    lg300 = (4.0 * rng.standard_normal(300)).astype(F)
    lg1500 = (4.0 * rng.standard_normal(1500)).astype(F)
    dry = dict(dry_multiplier=0.8, dry_base=1.75, dry_allowed_length=2, seq_last_n=1024)
    base7 = [1, 2, 3, 9, 1, 2, 3]          # the suffix 1 2 3 occurred before, followed by 9: rep_9 = ng_9 = 3
    out["window_0"] = (300, lg300, [], dict(dry, no_repeat_ngram=2), {}, {})
    out["window_1"] = (300, lg300, [5], dict(dry, no_repeat_ngram=2), {}, {})
    out["window_2"] = (300, lg300, [5, 5], dict(dry, dry_allowed_length=1, no_repeat_ngram=2), {}, {5: (1, 1)})
    per = ([11, 12, 13, 14, 15, 16, 17] * 147)
    out["window_1023"] = (300, lg300, per[:1023], dict(dry, no_repeat_ngram=64), {}, None)
    out["window_1024"] = (300, lg300, per[:1024], dict(dry, no_repeat_ngram=64), {}, None)
    out["window_over_ring"] = (300, lg300, per + per[:5], dict(dry, no_repeat_ngram=3), {}, None)
    out["last_n_shorter"] = (300, lg300, [4, 8] * 60 + base7, dict(dry, seq_last_n=5), {}, {9: (1, 1)})
    out["aaaaa"] = (300, lg300, [7] * 5, dry, {}, {7: (4, 4)})
    out["period_3"] = (300, lg300, [1, 2, 3] * 5, dry, {}, {1: (12, 12)})
    out["match_cap"] = (300, lg300, [9] * 100, dict(dry, dry_multiplier=0.01, dry_base=1.2), {}, {9: (64, 64)})
    out["max_of_two"] = (300, lg300, [1, 2, 3, 9, 5, 3, 9, 1, 2, 3], dry, {}, {9: (3, 3)})
    out["below_allowed"] = (300, lg300, base7, dict(dry, dry_allowed_length=4), {}, {9: (3, 3)})
    out["at_allowed"] = (300, lg300, base7, dict(dry, dry_allowed_length=3), {}, {9: (3, 3)})
    out["breaker_in_suffix"] = (300, lg300, base7, dict(dry, breakers=(2,)), {}, {9: (1, 3)})
    out["breaker_last"] = (300, lg300, base7, dict(dry, breakers=(3, 250)), {}, {9: (0, 3)})
    w = [1100, 1200, 1300, 1400, 1100, 1200, 1300]
    out["breakers_1024"] = (1500, lg1500, w, dict(dry, breakers=tuple(range(177, 1201))), {}, {1400: (1, 3)})
    out["bias_neg_inf"] = (300, lg300, base7, dry, dict(logit_bias=[(9, NEG_INF), (40, -1.5)]), {9: (3, 3)})
    out["in_penalty_window"] = (300, lg300, base7, dry, dict(X.ALL3, last_n=4, logit_bias=[(9, 0.75)]), {9: (3, 3)})
    out["overflow"] = (300, lg300, base7, dict(dry, dry_multiplier=BIG, dry_base=1e10, dry_allowed_length=1), {}, {9: (3, 3)})
    out["ngram_2"] = (300, lg300, [3, 9, 5, 3, 8, 3], dict(no_repeat_ngram=2, seq_last_n=1024), {}, {9: (1, 1), 8: (1, 1)})
    out["ngram_64"] = (300, lg300, per[:200], dict(no_repeat_ngram=64, seq_last_n=1024), {}, None)
    out["ngram_longer_than_window"] = (300, lg300, [1, 2, 1, 2, 1], dict(no_repeat_ngram=10, seq_last_n=1024), {}, {2: (3, 3)})
    for v in out.values():
        v[1].setflags(write=False)
    return out


def edge_expected(name):
    """(l' after the stages, rep, ng) of a named case."""
    V, lg, win, seq, ctl, _ = edge_cases()[name]
    return seq_adjust(X.adjust(lg, win, **ctl), win, **seq)


def empty_vocabulary_case():
    """(logits, window, seq controls, logit_ctl controls) at V = 300: 256 -inf biases and a ban on the
    44 other tokens, each of which has followed the last token: no finite logit is left."""
    V = 300
    lg = np.ascontiguousarray(logits(V))
    free = list(range(256, 300))
    t = free[0]
    win = [t, t]
    for c in free[1:]:
        win += [c, t]
    return lg, win, dict(no_repeat_ngram=2, seq_last_n=1024), dict(logit_bias=[(i, NEG_INF) for i in range(256)])


def xtc_edge_cases():
    """name -> (logits, SeqAnalysis kwargs, |A| expected, kept ids of a fired draw or None), V = 300:
    every one must be decided."""
    V = 300
    rng = np.random.default_rng(37)
    out = {}
    flat = np.zeros(V, F)
    out["a_0"] = (flat.copy(), dict(temperature=1.0, xtc_probability=1.0, xtc_threshold=0.5), 0, list(range(V)))
    lg = np.full(V, -4.0, F)
    lg[21] = 6.0
    out["a_1"] = (lg, dict(temperature=1.0, xtc_probability=1.0, xtc_threshold=0.3), 1, list(range(V)))
    lg = np.full(V, -4.0, F)
    lg[[21, 200]] = 6.0, 5.5
    out["a_2"] = (lg, dict(temperature=1.0, xtc_probability=1.0, xtc_threshold=0.2), 2, [i for i in range(V) if i != 21])
    out["a_all"] = (flat.copy(), dict(temperature=1.0, xtc_probability=1.0, xtc_threshold=1e-3), V, [V - 1])
    lg = np.full(V, -4.0, F)
    lg[7] = 6.0
    lg[[33, 150, 151]] = 5.0               # equal keys at the bottom of A: the highest index survives
    out["tie_at_bottom"] = (lg, dict(temperature=1.0, xtc_probability=1.0, xtc_threshold=0.1), 4,
                            [i for i in range(V) if i not in (7, 33, 150)])
    lg = np.full(V, -4.0, F)
    lg[[5, 6, 7, 8, 9]] = 6.0, 5.5, 5.0, 4.5, 4.0
    out["top_k_partial"] = (lg, dict(temperature=1.0, top_k=3, xtc_probability=1.0, xtc_threshold=0.15), 3, [7])
    lg = (3.0 * rng.standard_normal(V)).astype(F)
    out["half_probability"] = (lg, dict(temperature=0.8, xtc_probability=0.5, xtc_threshold=0.05), None, None)
    # the typical stage drops the dominant token and keeps 170 of the flat tail plus the runner-ups:
    # C is no prefix of the order
    lg = np.zeros(V, F)
    lg[0] = F(np.log(40.0))
    lg[[1, 2]] = 0.5, 0.25
    out["behind_typical"] = (lg, dict(temperature=1.0, typical_p=0.5, xtc_probability=1.0, xtc_threshold=0.007), None, None)
    lg = (3.0 * rng.standard_normal(V)).astype(F)
    out["top_p_behind"] = (lg, dict(temperature=1.2, top_p=0.8, xtc_probability=1.0, xtc_threshold=0.04), None, None)
    for v in out.values():
        v[0].setflags(write=False)
    return out


@lru_cache(maxsize=None)
def xtc_edge_analysis(name):
    lg, kw, _, _ = xtc_edge_cases()[name]
    kw = dict(kw)
    return SeqAnalysis(lg, kw.pop("temperature"), **kw)
