"""The decode entries as tables: invalid calls of the six xh_decode_* and the five xh_op_sample*
entries with what decides their report (one argument wrong, or two where the order of the checks
picks the message), and one interleaved run of all six heads on a context.

tests/golden/make_decode_entry_fixtures.py records both from the library _lib loads (the parent
commit's build, once); test_decode_entries_cpu.py and test_decode_heads_gpu.py replay them on the
current build and compare codes, texts and bits."""
import ctypes

import numpy as np

from xalm_amd import _lib as L

NAN, INF = float("nan"), float("inf")
NULL = "null"   # a pointer argument passed as null
V = 64          # the ops' vocabulary
SAMPLING = (1.0, 0, 1.0, 1)
TRUNC = (1.0, 0.0, 0.0, 0.1)
DECODE = ("greedy", "sample", "ext", "dfa", "adapt", "seq")
OPS = ("sample", "ext", "dfa", "adapt", "seq")


def _struct(cls, v):
    return None if v == NULL else ctypes.byref(v if isinstance(v, cls) else cls(*v))


def _ctl(ctl):
    """(pointer, keep-alive) of ctl: None = no controls, a dict of L.logit_ctl's arguments, or an XhLogitCtl"""
    if ctl is None:
        return None, None
    if isinstance(ctl, L.XhLogitCtl):
        return ctypes.byref(ctl), ctl
    c, keep = L.logit_ctl(**ctl)
    return ctypes.byref(c), (c, keep)


def _seq(seq):
    if seq == NULL:
        return None, None
    if isinstance(seq, L.XhSeqCtl):
        return ctypes.byref(seq), seq
    q, keep = L.seq_ctl(**(seq or {}))
    return ctypes.byref(q), (q, keep)


def _tokens(toks, n):
    """(pointer, count) of a token list; n overrides the count (a negative one, or one with a null list)"""
    a = np.ascontiguousarray(toks if toks is not None else [], dtype=np.int32)
    return (L.ptr(a) if a.size else None), (a.size if n is None else n), a


def prime(lib, ctx=None):
    """Leave a known text in the error slot a call reports to, so a bare return code shows as that text kept."""
    if ctx is None:
        lib.xh_philox4x32(0, 0, None)
    else:
        lib.xh_forward(ctx, -1, 0, L.OUTPUT_LOGITS, None)


def last_error(lib, ctx=None):
    return (lib.xh_last_error(ctx) or b"").decode()


def decode_call(lib, entry, ctx=None, pos=0, n_steps=4, sampling=SAMPLING, ctl=None, trunc=TRUNC, seq=None, history=None,
                n_history=None, constrain=0, state=0, mu=0.0, stop=(-1, -1)):
    """One xh_decode_<entry> call -> [return code, the error text after it, *n_done (-7 before the call)]."""
    prime(lib, ctx)
    n = max(n_steps, 1) if n_steps <= 64 else 1   # an n_steps past the cap is rejected before anything is written
    toks, lps = np.zeros(n, np.int32), np.zeros(n, np.float32)
    done, st, mu_out = ctypes.c_int(-7), ctypes.c_uint32(0), ctypes.c_float(0)
    s, t = _struct(L.XhSampling, sampling), _struct(L.XhTruncCtl, trunc)
    c, keep_c = _ctl(ctl)
    q, keep_q = _seq(seq)
    h, nh, keep_h = _tokens(history, n_history)
    tail = (stop[0], stop[1], L.ptr(toks))
    d = ctypes.byref(done)
    if entry == "greedy":
        rc = lib.xh_decode_greedy(ctx, pos, n_steps, *tail, d)
    elif entry == "sample":
        rc = lib.xh_decode_sample(ctx, pos, n_steps, s, *tail, d)
    elif entry == "ext":
        rc = lib.xh_decode_sample_ext(ctx, pos, n_steps, s, c, h, nh, *tail, L.ptr(lps), d)
    elif entry == "dfa":
        rc = lib.xh_decode_sample_dfa(ctx, pos, n_steps, s, c, h, nh, state, *tail, L.ptr(lps), ctypes.byref(st), d)
    elif entry == "adapt":
        rc = lib.xh_decode_sample_adapt(ctx, pos, n_steps, s, c, t, h, nh, constrain, state, mu, *tail, L.ptr(lps),
                                        ctypes.byref(st), ctypes.byref(mu_out), d)
    else:
        rc = lib.xh_decode_sample_seq(ctx, pos, n_steps, s, c, t, q, h, nh, constrain, state, mu, *tail, L.ptr(lps),
                                      ctypes.byref(st), ctypes.byref(mu_out), d)
    del keep_c, keep_q, keep_h
    return [int(rc), last_error(lib, ctx), int(done.value)]


def good_dfa():
    """One accepting state that reads every byte, over V one-byte pieces."""
    return L.ByteDfa(np.zeros((1, 256), np.uint16), np.ones(1, np.uint8)), L.pieces_blob([bytes([65 + i % 26]) for i in range(V)])


def op_call(lib, entry, vocab=V, logits=True, sampling=SAMPLING, ctl=None, trunc=TRUNC, seq=None, window=None, n_window=None,
            dfa="good", n_states=None, pieces=True, offset0=0, state=0, mu=0.0, stop=(-1, -1), n_draws=4, null_out=()):
    """One xh_op_sample<_entry> call that the argument checks reject -> [return code, the error text].
    dfa: "good" (where the entry takes one), None, or NULL for xh_op_sample_dfa's; n_states overrides its
    count, pieces False passes null tables, offset0 is offsets[0]; null_out names outputs passed as null."""
    prime(lib)
    nd = max(min(n_draws, 8), 1)
    lg = np.zeros(max(min(vocab, V), 1), np.float32)
    out = {k: np.zeros(nd, dt) for k, dt in (("tokens", np.int32), ("n_kept", np.int32), ("states", np.uint32),
                                             ("mu", np.float32))}
    o = {k: (None if k in null_out else L.ptr(a)) for k, a in out.items()}
    s, t = _struct(L.XhSampling, sampling), _struct(L.XhTruncCtl, trunc)
    c, keep_c = _ctl(ctl)
    q, keep_q = _seq(seq)
    w, nw, keep_w = _tokens(window, n_window)
    d, (blob, offsets) = good_dfa()
    offsets[0] = offset0
    use_dfa = dfa == "good" and entry in ("dfa", "adapt", "seq")
    dp = ctypes.byref(d.abi(n_states)) if use_dfa else None
    bp, op = (L.ptr(blob), L.ptr(offsets)) if use_dfa and pieces else (None, None)
    lp = L.ptr(lg) if logits else None
    if entry == "sample":
        rc = lib.xh_op_sample(lp, vocab, s, 0, n_draws, o["tokens"], o["n_kept"])
    elif entry == "ext":
        rc = lib.xh_op_sample_ext(lp, vocab, s, c, w, nw, 0, n_draws, o["tokens"], o["n_kept"], None, None)
    elif entry == "dfa":
        rc = lib.xh_op_sample_dfa(lp, vocab, s, c, w, nw, dp, bp, op, state, stop[0], stop[1], 0, n_draws, o["tokens"],
                                  o["n_kept"], None, o["states"], None)
    elif entry == "adapt":
        rc = lib.xh_op_sample_adapt(lp, vocab, s, c, t, w, nw, dp, bp, op, state, mu, stop[0], stop[1], 0, n_draws,
                                    o["tokens"], o["n_kept"], o["states"], o["mu"], None, None)
    else:
        rc = lib.xh_op_sample_seq(lp, vocab, s, c, t, q, w, nw, dp, bp, op, state, mu, stop[0], stop[1], 0, n_draws,
                                  o["tokens"], o["n_kept"], o["states"], o["mu"], None, None, None, None, None)
    del keep_c, keep_q, keep_w
    return [int(rc), last_error(lib)]


# ---- the context-free table ------------------------------------------------------------------------
BAD_SAMPLING = {"temperature<0": (-1.0, 0, 1.0, 1), "temperature nan": (NAN, 0, 1.0, 1), "top_k<0": (1.0, -1, 1.0, 1),
                "top_p 0": (1.0, 0, 0.0, 1), "top_p>1": (1.0, 0, 1.5, 1), "null sampling": NULL}
BAD_CTL = {"repeat_penalty 0": dict(repeat_penalty=0.0), "presence inf": dict(presence_penalty=INF),
           "last_n>max": dict(last_n=L.CTL_MAX_WINDOW + 1), "min_p>1": dict(min_p=1.5),
           "n_bias<0": L.XhLogitCtl(1.0, 0.0, 0.0, 0, 0.0, -1, None, None),
           "null bias": L.XhLogitCtl(1.0, 0.0, 0.0, 0, 0.0, 2, None, None),
           "bias id<0": dict(logit_bias=[(-1, 0.5)]), "bias dup": dict(logit_bias=[(3, 0.5), (3, 1.0)]),
           "bias +inf": dict(logit_bias=[(3, INF)])}
BAD_TOKENS = {"count<0": dict(toks=None, n=-1), "null list": dict(toks=None, n=3), "token<0": dict(toks=[1, -2, 3], n=None)}
BAD_TRUNC = {"null trunc": NULL, "typical_p 0": (0.0, 0.0, 0.0, 0.1), "sigma<0": (1.0, -1.0, 0.0, 0.1),
             "tau nan": (1.0, 0.0, NAN, 0.1), "eta 0": (1.0, 0.0, 3.0, 0.0), "miro+typical": (0.5, 0.0, 3.0, 0.1)}
BAD_SEQ = {"null seq": NULL, "dry_multiplier<0": dict(dry_multiplier=-0.1), "dry_base<1": dict(dry_base=0.5),
           "allowed 0": dict(dry_allowed_length=0), "ngram 1": dict(no_repeat_ngram=1),
           "null breakers": L.XhSeqCtl(0.8, 1.75, 2, 0, 64, 3, None, 0.0, 0.1), "breaker dup": dict(breakers=(5, 5)),
           "xtc_p>1": dict(xtc_probability=1.5), "xtc_thr 0": dict(xtc_threshold=0.0)}
MIRO = (1.0, 0.0, 3.0, 0.1)


def _from(entries, first):
    return entries[entries.index(first):]


def cpu_cases():
    """[(id, "decode" | "op", entry, arguments)]: every call is rejected before it touches a device."""
    rows = []
    for e in DECODE:
        # a null context and a negative step count return the bare code; the sampled entries have
        # zeroed *n_done by then, xh_decode_greedy has not
        rows += [(f"decode {e}: null ctx", "decode", e, {}), (f"decode {e}: n_steps<0", "decode", e, dict(n_steps=-1)),
                 (f"decode {e}: pos<0, null ctx", "decode", e, dict(pos=-1))]
    for e in _from(DECODE, "sample"):
        rows += [(f"decode {e}: {k}", "decode", e, dict(sampling=v)) for k, v in BAD_SAMPLING.items()]
        rows.append((f"decode {e}: sampling before n_steps", "decode", e, dict(sampling=BAD_SAMPLING["top_p 0"], n_steps=-1)))
    for e in _from(DECODE, "ext"):
        rows += [(f"decode {e}: {k}", "decode", e, dict(ctl=v)) for k, v in BAD_CTL.items()]
        rows += [(f"decode {e}: history {k}", "decode", e, dict(history=v["toks"], n_history=v["n"])) for k, v in BAD_TOKENS.items()]
        rows += [(f"decode {e}: sampling before ctl", "decode", e, dict(sampling=NULL, ctl=BAD_CTL["min_p>1"])),
                 (f"decode {e}: history before ctl", "decode", e, dict(history=[-1], ctl=BAD_CTL["min_p>1"])),
                 (f"decode {e}: ctl before n_steps", "decode", e, dict(ctl=BAD_CTL["min_p>1"], n_steps=-1))]
    for e in _from(DECODE, "adapt"):
        rows += [(f"decode {e}: {k}", "decode", e, dict(trunc=v)) for k, v in BAD_TRUNC.items()]
        rows += [(f"decode {e}: mu<0", "decode", e, dict(trunc=MIRO, mu=-1.0)),
                 (f"decode {e}: miro+top_k", "decode", e, dict(trunc=MIRO, mu=6.0, sampling=(1.0, 40, 1.0, 1))),
                 (f"decode {e}: miro+min_p", "decode", e, dict(trunc=MIRO, mu=6.0, ctl=dict(min_p=0.1))),
                 (f"decode {e}: ctl before trunc", "decode", e, dict(ctl=BAD_CTL["bias dup"], trunc=NULL)),
                 (f"decode {e}: trunc before n_steps", "decode", e, dict(trunc=BAD_TRUNC["sigma<0"], n_steps=-1)),
                 (f"decode {e}: trunc before constraint", "decode", e, dict(trunc=NULL, constrain=1, state=9))]
    rows += [(f"decode seq: {k}", "decode", "seq", dict(seq=v)) for k, v in BAD_SEQ.items()]
    rows += [("decode seq: miro+xtc", "decode", "seq", dict(trunc=MIRO, mu=6.0, seq=dict(xtc_probability=0.5))),
             ("decode seq: trunc before seq", "decode", "seq", dict(trunc=BAD_TRUNC["typical_p 0"], seq=NULL)),
             ("decode seq: seq before n_steps", "decode", "seq", dict(seq=NULL, n_steps=-1))]

    for e in OPS:
        rows += [(f"op {e}: {k}", "op", e, dict(sampling=v)) for k, v in BAD_SAMPLING.items()]
        rows += [(f"op {e}: null logits", "op", e, dict(logits=False)), (f"op {e}: vocab 0", "op", e, dict(vocab=0)),
                 (f"op {e}: vocab>max", "op", e, dict(vocab=(1 << 17) + 1)), (f"op {e}: n_draws 0", "op", e, dict(n_draws=0)),
                 (f"op {e}: n_draws>max", "op", e, dict(n_draws=65537)),
                 (f"op {e}: null tokens_out", "op", e, dict(null_out=("tokens",))),
                 (f"op {e}: null n_kept_out", "op", e, dict(null_out=("n_kept",))),
                 (f"op {e}: sampling before args", "op", e, dict(sampling=NULL, logits=False))]
    for e in _from(OPS, "ext"):
        rows += [(f"op {e}: {k}", "op", e, dict(ctl=v)) for k, v in BAD_CTL.items()]
        rows += [(f"op {e}: window {k}", "op", e, dict(window=v["toks"], n_window=v["n"])) for k, v in BAD_TOKENS.items()]
        rows += [(f"op {e}: window token>=vocab", "op", e, dict(window=[1, V])),
                 (f"op {e}: bias id>=vocab", "op", e, dict(ctl=dict(logit_bias=[(V, 0.5)]))),
                 (f"op {e}: args before ctl", "op", e, dict(n_draws=0, ctl=BAD_CTL["min_p>1"]))]
    for e in _from(OPS, "dfa"):
        # next_state_out is required from here on; the constraint is xh_op_sample_dfa's own and optional above it
        rows += [(f"op {e}: null next_state_out", "op", e, dict(null_out=("states",))),
                 (f"op {e}: n_states 0", "op", e, dict(n_states=0)), (f"op {e}: null pieces", "op", e, dict(pieces=False)),
                 (f"op {e}: offsets[0] 1", "op", e, dict(offset0=1)), (f"op {e}: state out of range", "op", e, dict(state=1)),
                 (f"op {e}: stop>=vocab", "op", e, dict(stop=(-1, V))),
                 (f"op {e}: ctl before dfa", "op", e, dict(ctl=BAD_CTL["last_n>max"], n_states=0)),
                 (f"op {e}: dfa before pieces", "op", e, dict(n_states=0, pieces=False)),
                 (f"op {e}: pieces before state", "op", e, dict(pieces=False, state=1)),
                 (f"op {e}: state before stop", "op", e, dict(state=1, stop=(V, -1)))]
    rows.append(("op dfa: null dfa", "op", "dfa", dict(dfa=NULL)))
    for e in _from(OPS, "adapt"):
        rows += [(f"op {e}: null mu_out", "op", e, dict(null_out=("mu",)))]
        rows += [(f"op {e}: {k}", "op", e, dict(trunc=v)) for k, v in BAD_TRUNC.items()]
        rows += [(f"op {e}: mu nan", "op", e, dict(trunc=MIRO, mu=NAN)),
                 (f"op {e}: ctl before trunc", "op", e, dict(ctl=BAD_CTL["n_bias<0"], trunc=BAD_TRUNC["tau nan"])),
                 (f"op {e}: trunc before dfa", "op", e, dict(trunc=BAD_TRUNC["eta 0"], n_states=0)),
                 (f"op {e}: no dfa, trunc", "op", e, dict(dfa=None, trunc=BAD_TRUNC["sigma<0"], state=1, stop=(V, V)))]
    rows += [(f"op seq: {k}", "op", "seq", dict(seq=v)) for k, v in BAD_SEQ.items()]
    rows += [("op seq: breaker>=vocab", "op", "seq", dict(seq=dict(breakers=(V,)))),
             ("op seq: trunc before seq", "op", "seq", dict(trunc=NULL, seq=NULL)),
             ("op seq: seq before dfa", "op", "seq", dict(seq=BAD_SEQ["ngram 1"], state=1))]
    assert len({r[0] for r in rows}) == len(rows)
    return rows


def run_cpu_case(lib, kind, entry, kw):
    return decode_call(lib, entry, **kw) if kind == "decode" else op_call(lib, entry, **kw)


# ---- invalid calls on a live context ---------------------------------------------------------------
PAST_CAP = 1 << 20   # above every context's decode capacity


def live_cases(vocab, n_states):
    """[(id, entry, arguments, constraint uploaded)]: rejected calls on a hydrated context, and the calls of
    no steps that the same arguments make valid where an entry does not check them."""
    rows = []
    for e in DECODE:
        rows.append((f"{e}: n_steps>cap", e, dict(n_steps=PAST_CAP), False))
    for e in _from(DECODE, "sample"):
        rows += [(f"{e}: pos<0", e, dict(pos=-1), False), (f"{e}: pos before n_steps", e, dict(pos=-1, n_steps=PAST_CAP), False)]
    rows.append(("greedy: pos<0, no steps", "greedy", dict(pos=-1, n_steps=0), False))
    bad = dict(state=n_states, stop=(vocab, -1))
    for e, on, off in (("dfa", {}, None), ("adapt", dict(constrain=1), dict(constrain=0)), ("seq", dict(constrain=1), dict(constrain=0))):
        rows += [(f"{e}: no constraint", e, dict(on), False),
                 (f"{e}: n_steps before constraint", e, dict(on, n_steps=PAST_CAP), False),
                 (f"{e}: state out of range", e, dict(on, state=n_states), True),
                 (f"{e}: dead state, stop>=vocab", e, dict(on, state=L.DFA_DEAD, stop=(-1, vocab)), True),
                 (f"{e}: state before stop", e, dict(on, **bad), True),
                 (f"{e}: n_steps before state", e, dict(on, n_steps=PAST_CAP, **bad), True)]
        if off is not None:
            rows += [(f"{e}: unconstrained, no constraint, no steps", e, dict(off, n_steps=0, **bad), False),
                     (f"{e}: unconstrained, no steps", e, dict(off, n_steps=0, **bad), True)]
    assert len({r[0] for r in rows}) == len(rows)
    return rows


# ---- all six heads on one context ------------------------------------------------------------------
FIXTURE = "tiny_mistral_f16"
PROMPT = [1, 84, 262, 259, 90]
EOS = 2
PATTERN = r"(of|to)( (of|to)){5}[.?]"   # test_constraint_gpu.py's
STEPS = 4
CTL = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2, last_n=4)
HEAD_ORDER = ("greedy", "sample", "ext", "dfa", "adapt", "seq")


def open_model(constraint=False, graphs=True):
    """(model, state, DFA of PATTERN) on FIXTURE, the constraint uploaded or not"""
    from conftest import fixture_path
    from xalm_amd.model import InferenceState, Model
    from xalm_amd.xalm_file import XalmFile
    xf = XalmFile(fixture_path(FIXTURE + ".xalm"))
    gm = Model.from_xalm(xf)
    gm.set_graphs(graphs)
    dfa = L.regex_compile(PATTERN)
    if constraint:
        upload_constraint(gm, dfa)
    return gm, InferenceState(gm.config), dfa


def upload_constraint(gm, dfa):
    from conftest import fixture_path
    from xalm_amd.xalm_file import XalmFile
    gm.set_constraint_vocab(L.token_pieces(XalmFile(fixture_path(FIXTURE + ".xalm")).tokens()))
    gm.set_constraint(dfa)


def run_live_cases(gm, st, dfa):
    """{id: [code, text, n_done]} of live_cases on gm after the prompt: the rows without a constraint first,
    then the upload and the rest."""
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    out = {}
    cases = live_cases(gm.config.vocab_size, dfa.n_states)
    for uploaded in (False, True):
        if uploaded:
            upload_constraint(gm, dfa)
        out.update({cid: decode_call(L.lib(), entry, ctx=gm._ctx, **kw) for cid, entry, kw, needs in cases if needs == uploaded})
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


def run_heads(gm, st, dfa, top):
    """The prompt, then twelve calls of STEPS steps on gm: the six heads in HEAD_ORDER (adapt constrained
    from the state the dfa call left, seq unconstrained), then the six in reverse (dfa from the state the
    adapt call left, which runs Mirostat this time).  The first pass captures each head's graph, the second
    replays it.  -> one record per call: tokens, log-probability bits, final state, final mu bits, and with
    `top` the rows of xh_get_top_logprobs."""
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    hist = list(PROMPT)
    out = []
    state = dfa.start
    for i, head in enumerate(HEAD_ORDER + HEAD_ORDER[::-1]):
        second = i >= len(HEAD_ORDER)
        pos, seed = len(hist), 7 + i
        lps, st_out, mu = [], None, None
        if head == "greedy":
            toks = gm.decode_greedy(pos, STEPS)
        elif head == "sample":
            toks = gm.decode_sample(pos, STEPS, 0.9, 40, 0.95, seed)
        elif head == "ext":
            toks, lps = gm.decode_sample_ext(pos, STEPS, 0.9, 40, 0.95, seed, min_p=0.02, logit_bias={90: -1.0}, history=hist,
                                             logprobs=True, stop=(EOS, -1), **CTL)
        elif head == "dfa":
            toks, lps, st_out = gm.decode_sample_dfa(pos, STEPS, 1.1, state, seed=seed, history=hist, stop=(EOS, -1), **CTL)
        elif head == "adapt":
            kw = dict(mirostat_tau=3.0, mirostat_eta=0.2) if second else dict(top_k=40, typical_p=0.9, top_n_sigma=2.0)
            toks, lps, st_out, mu = gm.decode_sample_adapt(pos, STEPS, 1.1, seed=seed, constrain=True, state=state,
                                                           history=hist, stop=(EOS, -1), **kw, **CTL)
        else:
            toks, lps, st_out, mu = gm.decode_sample_seq(pos, STEPS, 1.2, 0, 0.95, seed, dry_multiplier=0.8, seq_last_n=64,
                                                         no_repeat_ngram=3, breakers=(13,), xtc_probability=0.5,
                                                         typical_p=0.95, history=hist, **CTL)
        if head in ("dfa", "adapt"):
            state = st_out
        rec = dict(head=head, tokens=list(toks), logprobs=bits(lps), state=st_out, mu=None if mu is None else bits([mu])[0])
        if top:
            ids, tl, rank = gm.top_logprobs(len(toks))
            rec["top"] = dict(ids=ids.tolist(), lps=[bits(r) for r in tl], rank=rank.tolist())
        out.append(rec)
        hist += list(toks)
        if not second and head == "seq":
            state = dfa.start   # the second pass constrains anew
    return out
