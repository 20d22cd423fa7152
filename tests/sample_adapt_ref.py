"""Reference for the adaptive draw (xh_trunc_ctl, include/xalm_hip.h), on top of sample_ref and
sample_ext_ref: top-n-sigma, the locally typical stage and Mirostat v2 in numpy float64 over exact
Python / int64 integer masses, and the case lists the CPU and GPU tests share.

The masses are the device's: M_i = trunc(f32 exp(f32((l_i - m) / T)) * 2^40), with numpy's float32
exp.  A device expf that differs from it by an ulp or two moves a mass by 2^-22 relative at most.

A case is undecided (skipped; at most sample_ref.SKIP_CAP of a grid, none of the named edge cases)
when one of these holds:
  - n-sigma: a finite logit other than the maximum lies within 4 f32 ulps of thr, which is rounded
    once from the float64 value;
  - typical, order: at the cut token c (the last one kept in the order of d) another token with mass
    has a float64 d within BAND(c, j) of d_c.  All tokens before c are then before it in any
    arithmetic, no prefix of them reaches the target, and c closes it: the kept set does not depend
    on the order among them;
  - typical, mass: the integer mass before c, or that mass plus M_c, lies within DELTA * S of
    ceil(typical_p * S);
  - Mirostat: a mass lies within MIRO_REL relative of the cut;
  - sample_ref's top-p band or sample_ext_ref's min-p band fires.

The band on d.  On the device p = (float)M / (float)S is three roundings, 3 * 2^-24 relative, and M
itself carries expf's 2^-22, so -ln p is off by at most 2^-21 absolute; logf adds 2 ulps of s, at
most 2^-22 |s|.  So |s - s64| <= EPS_S(s) = 2^-21 + 2^-22 max(1, |s|).  H is a fixed-order f32 sum of
up to V positive terms p s, each off by about 2^-21 relative: sample_ref's DELTA bounds the sum's
own error, so |H - H64| <= EPS_H = (DELTA + 2^-21) max(1, H).  H's error moves d of two tokens on
opposite sides of H in opposite directions, so two d can approach each other by 2 EPS_H:
BAND(c, j) = EPS_S(s_c) + EPS_S(s_j) + 2 EPS_H.  Nothing here is fitted to the device.

MIRO_REL = max(V * 2^-40, 2^-21): the issue's V * 2^-40 is the truncation of the masses in S; expf's
2^-22 on the mass and on S each add up to 2^-21, which is the larger for every vocabulary here.

mu' is compared with the float64 value within 8 f32 ulps of max(1, |mu|, |obs|, tau).
"""
from functools import lru_cache

import numpy as np

import sample_ext_ref as X
import sample_ref as R

F = np.float32
MASS_ONE = 2.0 ** 40
NEG_INF = float("-inf")


def masses(lg, T):
    """int64 [V]: the device's integer masses of the logits under temperature T (max finite)."""
    lg = np.ascontiguousarray(lg, dtype=F)
    m = lg.max()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        w = np.exp(((lg - m) / F(T)).astype(F)).astype(F)
        M = np.trunc(w.astype(np.float64) * MASS_ONE).astype(np.int64)
    M[np.isneginf(lg)] = 0
    return M


def eps_s(s):
    return 2.0 ** -21 + 2.0 ** -22 * max(1.0, abs(s))


def eps_h(H):
    return (R.DELTA + 2.0 ** -21) * max(1.0, H)


def mu_bound(mu, obs, tau):
    return 8 * 2.0 ** -23 * max(1.0, abs(mu), abs(obs), tau)


class AdaptAnalysis:
    """The adaptive draw on l'' (already adjusted and masked) at temperature > 0.
    kept_map uint8 [V]: the set after the typical stage and before top-p; thr: the n-sigma threshold
    (float32, -inf = off); final: the sample_ref.Analysis of the draw (kept, band, accepted);
    n_kept: the final kept set's size as the device reports it; reasons: why it is undecided."""

    def __init__(self, lpp, temperature, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, top_n_sigma=0.0, tau=0.0,
                 eta=0.1, mu=0.0):
        lg = np.ascontiguousarray(lpp, dtype=F)
        V = lg.size
        self.V, self.T, self.tau, self.eta, self.mu = V, float(F(temperature)), float(F(tau)), float(F(eta)), float(F(mu))
        self.reasons = []
        self.thr = NEG_INF
        self.K = None
        m = float(lg.max())
        if not np.isfinite(m):
            self.kept_map = np.zeros(V, np.uint8)
            self.final = R.Analysis(lg, temperature, 0, top_p)
            self.n_kept = 0
            return
        ext = X.ExtAnalysis(lg, temperature, top_k, 1.0, min_p)
        if ext.minp_band.size:
            self.reasons.append("min-p band")
        n = top_k if 0 < top_k < V else V
        if ext.n_minp is not None and 1 <= ext.n_minp < n:
            n = ext.n_minp
        ns = float(F(top_n_sigma))
        if ns > 0.0:
            fin = lg[np.isfinite(lg)].astype(np.float64)
            sigma = float(np.sqrt(((fin - fin.mean()) ** 2).mean()))
            thr = F(m - ns * sigma)
            self.thr = float(thr)
            near = np.isfinite(lg) & (np.abs(lg.astype(np.float64) - float(thr)) <= 4 * float(np.spacing(np.abs(thr)))) \
                & (lg != F(m))
            if near.any():
                self.reasons.append("n-sigma threshold")
            n_sigma = int((lg >= thr).sum())
            if 1 <= n_sigma < n:
                n = n_sigma
        M = masses(lg, self.T)
        self.M = M
        if self.tau > 0.0:
            S = int(M.sum())
            cut = int(np.ceil(S * 2.0 ** -self.mu))
            rel = max(V * 2.0 ** -40, 2.0 ** -21)
            if (np.abs(M.astype(np.float64) - cut) <= rel * cut + 1).any() and cut > 0:
                self.reasons.append("Mirostat cut")
            n = max(1, int((M >= cut).sum()))
        self.n_prefix = n
        order = np.lexsort((np.arange(V), R.M32 - R.order_keys(lg).astype(np.int64)))[:n]
        P = float(F(typical_p))
        if P < 1.0:
            self.kept_map = self._typical(lg, M, order, P)
            cutlg = np.where(self.kept_map.astype(bool), lg, F(NEG_INF)).astype(F)
            self.final = R.Analysis(cutlg, temperature, 0, top_p)
            self.n_kept = self.final.n_kept if float(F(top_p)) < 1.0 else int(self.kept_map.sum())
        else:
            self.kept_map = np.zeros(V, np.uint8)
            self.kept_map[order] = 1
            self.final = R.Analysis(lg, temperature, n if n < V else 0, top_p)
            self.n_kept = self.final.n_kept
        if self.final.band.size:
            self.reasons.append("top-p band")
        if self.tau > 0.0:
            self.K = int(M[self.kept_map.astype(bool)].sum())

    def _typical(self, lg, M, order, P):
        V = lg.size
        c_ids = np.sort(order)
        c_ids = c_ids[M[c_ids] > 0]
        Mc = M[c_ids]
        S = int(Mc.sum())
        p = Mc.astype(np.float64) / S
        s = -np.log(p)
        H = float((p * s).sum())
        d = np.abs(s - H)
        by_d = np.lexsort((c_ids, d))
        cum = np.cumsum(Mc[by_d])
        target = min(max(int(np.ceil(P * S)), 1), S)
        c = int(np.searchsorted(cum, target, side="left"))  # the first position whose prefix reaches it
        kept = np.zeros(V, np.uint8)
        kept[c_ids[by_d[: c + 1]]] = 1
        # bands
        jc = by_d[c]
        band = eps_s(s[jc]) + np.array([eps_s(x) for x in s]) + 2 * eps_h(H)
        close = np.abs(d - d[jc]) <= band
        close[jc] = False
        # equal float64 d with a different index is a tie the index decides only if the f32 d are
        # equal too: equal masses give equal p, s and d in any arithmetic
        close &= ~(Mc == Mc[jc])
        if close.any():
            self.reasons.append("typical order")
        before = int(cum[c - 1]) if c > 0 else 0
        # (nothing precedes the first token: an empty prefix is exact)
        if (c > 0 and abs(before - target) < R.DELTA * S) or abs(int(cum[c]) - target) < R.DELTA * S:
            if not (Mc == int(MASS_ONE)).all():  # all maxima: expf(0) = 1 in any arithmetic, the integers are exact
                self.reasons.append("typical mass")
        self.H, self.S = H, S
        return kept

    @property
    def decided(self):
        return not self.reasons

    def accepted(self, seed, pos):
        return self.final.accepted(seed, pos)

    def mu_next(self, token):
        """(float64 mu', obs) after `token` was drawn."""
        obs = float(np.log2(self.K) - np.log2(int(self.M[token])))
        return self.mu - self.eta * (obs - self.tau), obs


# ---- the case lists -------------------------------------------------------------------------
# peaked_logits' own seed gives at most SKIP_CAP undecided grid cases at both vocabularies
# (test_sample_adapt_cpu.py checks it), so no other seed is needed.
VOCABS = (300, 128256)


def grid():
    """(temperature, top_k, typical_p, top_n_sigma, top_p) of the op test."""
    return [(t, k, ty, ns, p) for t in (0.7, 1.5) for k in (0, 40) for ty in (1.0, 0.9, 0.2) for ns in (0.0, 1.0)
            for p in (1.0, 0.9)]


@lru_cache(maxsize=None)
def grid_analysis(V, t, k, ty, ns, p):
    return AdaptAnalysis(R.peaked_logits(V), t, top_k=k, top_p=p, typical_p=ty, top_n_sigma=ns)


def miro_grid():
    """(temperature, tau, eta, mu) of Mirostat's op test."""
    return [(t, tau, 0.1, mu) for t in (0.7, 1.5) for tau in (3.0, 5.0) for mu in (2.0, 6.0, 10.0)]


@lru_cache(maxsize=None)
def miro_analysis(V, t, tau, eta, mu):
    return AdaptAnalysis(R.peaked_logits(V), t, tau=tau, eta=eta, mu=mu)


BAN = [(12, NEG_INF), (8, NEG_INF), (40, NEG_INF)]


def edge_cases():
    """name -> (logits, kwargs of AdaptAnalysis, logit_ctl controls, expected kept ids or None), V = 300:
    every one must be decided.  The controls (biases only) are applied by sample_ext_ref.adjust."""
    V = 300
    rng = np.random.default_rng(23)
    out = {}
    # one dominant token over a flat tail: p_0 = 40 / 339, s_0 = 2.14, tail s = 5.83, H = 5.39, so
    # d_0 = 3.25 against the tail's 0.44: the tail comes first, 170 of its tokens reach half the mass
    lg = np.full(V, 0.0, F)
    lg[0] = F(np.log(40.0))
    out["typical_drops_argmax"] = (lg, dict(temperature=1.0, typical_p=0.5), {}, list(range(1, 171)))
    lg = (8.0 * rng.standard_normal(V)).astype(F)
    out["typical_keeps_one"] = (lg, dict(temperature=0.7, typical_p=1e-6), {}, None)
    out["typical_all_equal"] = (np.full(V, 1.25, F), dict(temperature=1.0, typical_p=0.25), {}, list(range(75)))
    lg = (4.0 * rng.standard_normal(V)).astype(F)
    lg[64:128] = -np.inf
    lg[130:140] = -200.0               # finite, but expf underflows the 2^-40 grid: M = 0
    out["typical_neg_inf_and_massless"] = (lg, dict(temperature=1.0, typical_p=0.9), {}, None)
    lg = np.full(V, -3.0, F)
    lg[[17, 99, 250]] = 6.0            # sigma = 0.9: thr = 5.55
    out["n_sigma_keeps_maxima"] = (lg, dict(temperature=1.0, top_n_sigma=0.5), {}, [17, 99, 250])
    out["n_sigma_zero_sigma"] = (np.full(V, 2.5, F), dict(temperature=1.0, top_n_sigma=1.0), {}, list(range(V)))
    lg = (8.0 * rng.standard_normal(V)).astype(F)
    out["n_sigma_under_top_k"] = (lg, dict(temperature=1.0, top_n_sigma=1.0, top_k=3), {}, None)
    out["min_p_under_n_sigma"] = (lg.copy(), dict(temperature=1.0, top_n_sigma=0.25, min_p=1e-9), {}, None)
    out["mirostat_mu_small"] = (lg.copy(), dict(temperature=1.0, tau=3.0, eta=0.1, mu=0.0), {}, [int(lg.argmax())])
    out["mirostat_mu_large"] = (lg.copy(), dict(temperature=4.0, tau=3.0, eta=0.1, mu=60.0), {}, list(range(V)))
    lg = (8.0 * rng.standard_normal(V)).astype(F)
    lg[40] = 30.0                      # the banned argmax
    for name, kw in (("ban_typical", dict(temperature=0.7, typical_p=0.9)),
                     ("ban_n_sigma", dict(temperature=0.7, top_n_sigma=1.0)),
                     ("ban_mirostat", dict(temperature=0.7, tau=3.0, eta=0.1, mu=6.0))):
        out[name] = (lg.copy(), kw, dict(logit_bias=BAN), None)
    for v in out.values():
        v[0].setflags(write=False)
    return out


def edge_analysis(name):
    lg, kw, ctl, _ = edge_cases()[name]
    kw = dict(kw)
    t = kw.pop("temperature")
    return AdaptAnalysis(X.adjust(lg, (), **ctl), t, **kw)
