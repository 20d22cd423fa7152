"""Reference for the top-N log-probabilities (XH_TOP_MAX, include/xalm_hip.h) in numpy, and the case
list the CPU and GPU tests share.

Ids and ranks come from integers alone: the f32 bits mapped to the sampler's unsigned key (a larger
logit = a larger key, +0 above -0), sorted by (key descending, index ascending).  The
log-probabilities are float64, as sample_ext_ref.logprob64, and compared under its logprob_bound.
"""
from functools import lru_cache

import numpy as np

from sample_ext_ref import logprob_bound

NEG_INF = float("-inf")
VOCABS = (300, 1025, 128256)
N_TOPS = (1, 5, 32)
N_ROWS = (1, 3)


def keys(row):
    u = np.ascontiguousarray(row, dtype=np.float32).view(np.uint32).astype(np.uint64)
    neg = (u & np.uint64(0x80000000)) != 0
    return np.where(neg, ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def order(row):
    """Every index of the row in the order: key descending, then index ascending."""
    k = keys(row)
    return np.lexsort((np.arange(k.size), np.uint64(0xFFFFFFFF) - k))


def logprobs64(row):
    lg = np.ascontiguousarray(row, dtype=np.float32).astype(np.float64)
    m = lg.max()
    with np.errstate(divide="ignore"):
        return (lg - m) - np.log(np.exp(lg - m).sum())


def top(row, n_top, target=None):
    """(ids [n_top], float64 log-probabilities [n_top]), plus (target's float64 log-probability,
    target's rank) with a target."""
    o = order(row)
    lp = logprobs64(row)
    ids = o[:n_top].astype(np.int32)
    if target is None:
        return ids, lp[ids]
    return ids, lp[ids], float(lp[target]), int(np.flatnonzero(o == target)[0])


def check_rows(logits, n_top, targets, got, tag=""):
    """Assert the rows of `got` = (ids, lps[, target lps, ranks]) against the reference on `logits`:
    ids and ranks exactly, log-probabilities within logprob_bound (-inf exactly)."""
    logits = np.atleast_2d(logits)
    for r in range(logits.shape[0]):
        want = top(logits[r], n_top, None if targets is None else int(targets[r]))
        assert got[0][r].tolist() == want[0].tolist(), (tag, r, got[0][r], want[0])
        for j in range(n_top):
            _close(got[1][r][j], want[1][j], (tag, r, j))
        if targets is not None:
            _close(got[2][r], want[2], (tag, r, "target"))
            assert int(got[3][r]) == want[3], (tag, r, int(got[3][r]), want[3])


def _close(got, want, what):
    if np.isneginf(want):
        assert np.isneginf(got), (what, got, want)
    else:
        assert abs(float(got) - want) <= logprob_bound(want), (what, float(got), want, logprob_bound(want))


@lru_cache(maxsize=None)
def cases(V, n_rows):
    """name -> (logits [n_rows, V], targets [n_rows]): one row pattern per stage of the kernel a
    selection can go wrong in; every row of a case has the pattern under its own seed.  The targets
    walk over the maximum, a member of the tie block, a -inf token and an arbitrary one."""
    out = {}

    def rows(name, make, targets):
        lg = np.stack([make(np.random.default_rng(7000 + 131 * V + 17 * r + len(out)), r) for r in range(n_rows)])
        lg = np.ascontiguousarray(lg, dtype=np.float32)
        tg = np.array([targets(lg[r], r) for r in range(n_rows)], dtype=np.int32)
        lg.setflags(write=False)
        out[name] = (lg, tg)

    def normal(rng, r):
        return rng.standard_normal(V) * 3.0

    rows("normal", normal, lambda l, r: int(np.argmax(l)) if r == 0 else (r * 97) % V)

    # the cut lies inside one key: the lowest indices win; the target's rank is its index
    rows("all_equal", lambda rng, r: np.full(V, 1.25 + r), lambda l, r: (V - 1, 0, 40)[r % 3])

    def tie_block(rng, r):
        # 3 tokens above, then 40 equal ones (at scattered indices) straddling places 3 .. 42
        l = rng.standard_normal(V) - 8.0
        idx = rng.permutation(V)
        l[idx[:3]] = (9.0, 8.0, 7.5)
        l[idx[3:43]] = 5.5
        return l

    def in_block(l, r):
        blk = np.flatnonzero(l == np.float32(5.5))
        return int(blk[(0, blk.size - 1, blk.size // 2)[r % 3]])

    rows("tie_block", tie_block, in_block)

    def zeros(rng, r):
        # both signs, +0 and -0 interleaved: +0 sorts above -0
        l = rng.standard_normal(V) * 0.5
        z = rng.permutation(V)[:40]
        l[z[:20]] = 0.0
        l[z[20:]] = -0.0
        l[l > 0] = -l[l > 0] if r == 1 else l[l > 0]   # row 1: the zeros are the top of the order
        return l

    rows("signed_zeros", zeros, lambda l, r: int(np.flatnonzero(np.signbit(l) & (l == 0))[0]))

    # one sign and exponent: every key shares the top radix digit, and most the second
    rows("peaked_digit", lambda rng, r: 1.0 + rng.random(V) * 0.999, lambda l, r: int(np.argmax(l)) if r else int(np.argmin(l)))

    def mostly_inf(rng, r):
        l = np.full(V, NEG_INF)
        l[rng.permutation(V)[:3]] = (2.0, -1.0, 0.5)
        return l

    # fewer finite logits than n_top = 5: the -inf tokens follow by index; the target is one of them
    rows("mostly_neg_inf", mostly_inf, lambda l, r: int(np.flatnonzero(np.isneginf(l))[(0, -1, 7)[r % 3]]))

    # quantised logits: many small tie blocks all over the order
    rows("quantised", lambda rng, r: np.round(rng.standard_normal(V) * 4.0) / 2.0, lambda l, r: int(np.argmax(l)))
    return out
