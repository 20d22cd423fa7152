"""Reference for the constrained draw (xh_byte_dfa, include/xalm_hip.h) in numpy, on top of
sample_ext_ref: the piece walk, the allowed set and successor states, the masked logits l'', the
constrained-greedy rule written out, and sample_ext_ref's analysis of l'' for a sampled draw.  Also
the DFAs, piece tables and case lists the CPU and GPU tests share.

A sampled draw is compared exactly: ExtAnalysis.accepted gives the tokens whose cumulative-weight
interval, widened by sample_ref's DELTA, holds the draw; when that is one token the device must
return it, when it is two (the draw lies within rounding of a boundary) the draw is skipped, at
most SKIP_CAP = 2 % of a case's draws.  Cases are chosen so that the top-p / min-p cuts themselves
are decided (test_constraint_cpu asserts both with the reference alone).
"""
from functools import lru_cache

import numpy as np

import sample_ext_ref as X
import sample_ref as R

DEAD = 0xFFFF
SKIP_CAP = 0.02
NEG_INF = float("-inf")


# ---- the definition ----------------------------------------------------------------------------
def walk(next_table, state, piece):
    """Where the walk of `piece` from `state` ends, or DEAD (also for an empty piece)."""
    if state == DEAD or len(piece) == 0:
        return DEAD
    s = int(state)
    for b in piece:
        s = int(next_table[s, b])
        if s == DEAD:
            return DEAD
    return s


@lru_cache(maxsize=8)
def _matrix(pieces, width):
    """(lengths [V], bytes [V, width] of the pieces no longer than width), built once per table."""
    lens = np.array([len(p) for p in pieces])
    mat = np.zeros((len(pieces), width), dtype=np.int64)
    for t, p in enumerate(pieces):
        if len(p) <= width:
            mat[t, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    return lens, mat


def mask(next_table, accept, pieces, state, stop=(-1, -1)):
    """(allowed bool [V], successor uint16 [V]) in `state`: all walks at once, one byte position per
    numpy pass."""
    V = len(pieces)
    succ = np.full(V, DEAD, dtype=np.int64)
    if state != DEAD:
        width = 16  # longer pieces (few) take the scalar walk
        lens, mat = _matrix(tuple(pieces), width)
        cur = np.where((lens > 0) & (lens <= width), int(state), DEAD)
        nt = np.asarray(next_table, dtype=np.int64)
        for k in range(width):
            live = np.flatnonzero((cur != DEAD) & (lens > k))
            if live.size == 0:
                break
            cur[live] = nt[cur[live], mat[live, k]]
        for t in np.flatnonzero(lens > width):
            cur[t] = walk(next_table, state, pieces[t])
        succ = cur
        for t in stop:
            if 0 <= t < V:
                succ[t] = int(state) if accept[state] else DEAD
    return succ != DEAD, succ.astype(np.uint16)


def masked_logits(adjusted, allowed, state):
    """l'': l' where allowed, -inf elsewhere; nothing is masked in the stuck state."""
    adj = np.ascontiguousarray(adjusted, dtype=np.float32)
    if state == DEAD:
        return adj.copy()
    return np.where(allowed, adj, np.float32(NEG_INF)).astype(np.float32)


def stuck_token(stop):
    return stop[0] if stop[0] >= 0 else stop[1] if stop[1] >= 0 else 0


def constrained_greedy(adjusted, allowed):
    """The first token of the sampler's order (key descending, index ascending) among the allowed."""
    ids = np.flatnonzero(allowed)
    keys = R.order_keys(np.ascontiguousarray(adjusted, dtype=np.float32))[ids].astype(np.int64)
    return int(ids[np.argmax(keys)])  # argmax returns the first maximum: the lowest index


class Step:
    """One constrained draw's reference: stuck / greedy token / analysis of l''."""

    def __init__(self, adjusted, next_table, accept, pieces, state, stop, temperature, top_k, top_p, min_p):
        self.allowed, self.succ = mask(next_table, accept, pieces, state, stop)
        self.masked = masked_logits(adjusted, self.allowed, state)
        self.stuck = state == DEAD or not self.allowed.any()
        self.greedy = float(np.float32(temperature)) == 0.0
        self.an = None
        if self.stuck:
            self.token = stuck_token(stop)
            self.n_kept = 0
        elif self.greedy:
            self.token = constrained_greedy(adjusted, self.allowed)
            self.n_kept = 1
        else:
            self.an = X.ExtAnalysis(self.masked, temperature, top_k, top_p, min_p)
            self.n_kept = self.an.n_kept

    @property
    def decided(self):
        return self.an is None or self.an.decided

    def accepted(self, seed, pos):
        return {self.token} if self.an is None else self.an.accepted(seed, pos)

    def next_state(self, token):
        return DEAD if self.stuck else int(self.succ[token])


# ---- hand-made DFAs --------------------------------------------------------------------------------
A, B, C = ord("a"), ord("b"), ord("c")


@lru_cache(maxsize=None)
def dfa(name):
    """name -> (next uint16 [n, 256], accept uint8 [n]), read-only."""
    if name == "dfa3":      # (ab)*c?: 0 -a-> 1 -b-> 0, 0 -c-> 2; 2 accepts and has no way on
        n = 3
        nxt = np.full((n, 256), DEAD, dtype=np.uint16)
        nxt[0, A], nxt[1, B], nxt[0, C] = 1, 0, 2
        acc = np.array([1, 0, 1], dtype=np.uint8)
    elif name == "dfa700":  # a cycle: a -> i + 1, b -> i + 7 (mod 700); c only from multiples of 9
        n = 700
        i = np.arange(n)
        nxt = np.full((n, 256), DEAD, dtype=np.uint16)
        nxt[:, A] = (i + 1) % n
        nxt[:, B] = (i + 7) % n
        nxt[i % 9 == 0, C] = (i[i % 9 == 0] + 350) % n
        acc = (i % 5 == 0).astype(np.uint8)
    elif name == "chain":   # a{39999}: i -a-> i + 1; the last state accepts and has no way on
        n = 40000
        nxt = np.full((n, 256), DEAD, dtype=np.uint16)
        nxt[:-1, A] = np.arange(1, n)
        acc = np.zeros(n, dtype=np.uint8)
        acc[-1] = 1
    else:
        raise KeyError(name)
    nxt.setflags(write=False)
    acc.setflags(write=False)
    return nxt, acc


DFAS = ("dfa3", "dfa700", "chain")
STOP = (5, -1)   # token 5's piece walks nowhere: an end token is allowed whatever its piece
NO_STOP = (-1, -1)
# (state, stop) per DFA: an accepting state with stops set, one with no stops, a stuck state
# (accepting, no way on, no stops; and DEAD itself), a non-accepting state with stops set
STATES = {
    "dfa3": [(0, STOP), (0, NO_STOP), (1, STOP), (2, STOP), (2, NO_STOP), (DEAD, STOP), (DEAD, NO_STOP)],
    "dfa700": [(0, STOP), (0, NO_STOP), (250, NO_STOP), (300, STOP), (511, STOP), (699, NO_STOP), (693, (-1, 5))],
    "chain": [(0, NO_STOP), (250, STOP), (32767, NO_STOP), (39990, STOP), (39999, STOP), (39999, NO_STOP), (DEAD, (-1, 5))],
}
VOCABS = (97, 4097, 131072)


@lru_cache(maxsize=None)
def pieces(V):
    """Random pieces of 1 .. 9 bytes over abc, then by hand: a forbidden token 0, an empty piece, the
    end token's (forbidden letters), one of 300 bytes."""
    rng = np.random.default_rng(7000 + V)
    lens = rng.integers(1, 10, V)
    letters = rng.integers(0, 3, int(lens.sum())).astype(np.uint8) + A
    offs = np.concatenate(([0], np.cumsum(lens)))
    out = [letters[offs[t]:offs[t + 1]].tobytes() for t in range(V)]
    out[:12] = [b"zz", b"a", b"ab", b"c", b"", b"zz", b"a" * 300, b"aa", b"abc", b"b", b"aaaaaaaaa", b"ba"]
    return tuple(out)


def logits(V):
    return R.peaked_logits(V)


CTL_ON = dict(X.ALL3, last_n=64, logit_bias=[(1, NEG_INF), (2, 1.5), (7, -0.75)])
# (temperature, top_k, top_p, min_p, controls on)
DRAWS = [(0.0, 0, 1.0, 0.0, False), (0.0, 0, 1.0, 0.0, True), (0.8, 0, 1.0, 0.0, False), (0.8, 40, 0.9, 0.0, True),
         (1.3, 0, 0.95, 0.02, True)]


@lru_cache(maxsize=None)
def window(V):
    return tuple([1, 2, 2, 7, 9, 9, 9] + list(X.draw_window(V)[:57]))


@lru_cache(maxsize=None)
def adjusted(V, on):
    out = X.adjust(logits(V), window(V), **CTL_ON) if on else logits(V).copy()
    out.setflags(write=False)
    return out


def controls(on):
    return dict(CTL_ON) if on else {}


@lru_cache(maxsize=None)
def step(V, name, state, stop, draw):
    t, k, p, mp, on = draw
    nxt, acc = dfa(name)
    return Step(adjusted(V, on), nxt, acc, pieces(V), state, stop, t, k, p, mp)
