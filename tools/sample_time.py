#!/usr/bin/env python
"""Sampled against greedy decode on the device, timed side by side in one process.

For the synthetic Mistral-7B f16 (V = 32000) and Llama-3-8B f16 (V = 128256) shapes: a 32-token
prompt, then 128-step xh_decode_greedy and xh_decode_sample (temperature 0.8, top_k 40, top_p
0.95) calls in turn, six of each, every call from the same position; ms/step of both and their
difference.  Then the sampled step head's own device time (xh_time_kernel 6, HIP events) under
three parameter sets, and the extended step head's (xh_time_kernel 7, xh_decode_sample_ext) at the
first of them with its controls off, with a 64-token window, and with a 1024-token window and 256
biases.  The comparison is the greedy loop of the same process on the same box.

Then the constrained step head (xh_time_kernel 8, xh_decode_sample_dfa) next to the extended head
of the same run under the same parameters, with synthetic pieces of realistic lengths (1 .. 12
bytes, mean about 5) and two permissive DFAs under which every piece is walked to its end: `.*`
(one state: the table sits in LDS) and a 700-state cycle over every byte (walked from global
memory); and the ms/step and tok/s of 128-step xh_decode_sample_dfa and xh_decode_sample_ext
calls in turn.

With --top-logprobs 1 (profiles/top_logprobs_time.txt; --only-top 1 leaves the sections above
out): the top-N row kernel alone (xh_time_kernel 9) at n_top 1, 5 and 32; the extended loop's
ms/step under xh_set_top_logprobs 0, 5 and 32, the three in turn within every round; and xh_score
(n_top 0 and 5) against xh_perplexity over 2048 tokens, from a reset context each.

With --adapt 1 (profiles/sample_adapt_time.txt; --only-adapt 1 leaves the sections above out): the
adaptive step head (xh_time_kernel 10, xh_decode_sample_adapt) next to the extended head (7) of the
same process under the same sampling parameters, with the truncation off, top-n-sigma 1.0, typical_p
0.9, and Mirostat v2 (tau 5, eta 0.1; top_k 0 and top_p 1 as it requires, for both heads).

Run under a time limit:  timeout -k 10 600 python tools/sample_time.py
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
from xalm_amd import _lib as L  # noqa: E402
from xalm_amd.model import InferenceState, Model  # noqa: E402

PARAMS = (0.8, 40, 0.95)
HEAD_SETS = [("t 0.8 k 40 p 0.95", (0.8, 40, 0.95)), ("t 0.8 k 0 p 0.95", (0.8, 0, 0.95)), ("t 0.8 k 0 p 1", (0.8, 0, 1.0)),
             ("t 0 (greedy)", (0.0, 0, 1.0))]
PENALTIES = dict(repeat_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2)


def ext_sets(vocab):
    """(label, history, controls) of the extended head's rows."""
    hist64 = [(i * 7919) % vocab for i in range(48)] + [3] * 16
    hist1024 = [(i * 7919) % 4096 % vocab for i in range(1024)]
    bias = [(i * 101 % vocab, -1.0) for i in range(256)]
    return [("controls off", [], {}), ("window 64", hist64, dict(PENALTIES, last_n=64)),
            ("window 64 min_p 0.05", hist64, dict(PENALTIES, last_n=64, min_p=0.05)),
            ("window 1024 bias 256", hist1024, dict(PENALTIES, last_n=1024, logit_bias=bias))]


def synthetic_pieces(vocab):
    """Lower-case pieces of 1 .. 12 bytes, short ones most frequent (mean about 5), no newline."""
    rng = np.random.default_rng(vocab)
    lens = np.minimum(1 + rng.geometric(0.22, vocab), 12)
    letters = rng.integers(ord("a"), ord("z") + 1, int(lens.sum())).astype(np.uint8)
    offs = np.concatenate(([0], np.cumsum(lens)))
    return [letters[offs[t]:offs[t + 1]].tobytes() for t in range(vocab)]


def cycle_dfa(n):
    """n states, every byte leads from state i to i + 1 (mod n), every state accepts."""
    nxt = np.repeat(((np.arange(n) + 1) % n).astype(np.uint16)[:, None], 256, axis=1)
    return L.ByteDfa(nxt, np.ones(n, np.uint8))


def constrained_rows(m, c, n, args):
    t, k, p = PARAMS
    pieces = synthetic_pieces(c.vocab_size)
    m.set_constraint_vocab(pieces)
    print(f"  pieces: {sum(map(len, pieces)) / len(pieces):.2f} bytes mean, {max(map(len, pieces))} longest")
    for label, dfa in ((".* (1 state, LDS)", L.regex_compile(".*")), ("700-state cycle (global)", cycle_dfa(700))):
        m.set_constraint(dfa)
        m.decode_sample_ext(n, 1, t, k, p, seed=3)
        ext_us = m.time_kernel(7, args.head_iters)
        m.decode_sample_dfa(n, 1, t, dfa.start, k, p, seed=3)
        dfa_us = m.time_kernel(8, args.head_iters)
        print(f"  heads alone, t {t} k {k} p {p}, {label:<24}: extended {ext_us:8.2f} us   constrained {dfa_us:8.2f} us"
              f"   ({dfa_us - ext_us:+.2f} us)", flush=True)
        m.decode_sample_ext(n, 8, t, k, p, seed=1)  # both graphs exist and are warm
        m.decode_sample_dfa(n, 8, t, dfa.start, k, p, seed=1)
        ext, con = [], []
        for r in range(args.rounds):
            t0 = time.perf_counter()
            m.decode_sample_ext(n, args.steps, t, k, p, seed=r)
            t1 = time.perf_counter()
            toks, _, _ = m.decode_sample_dfa(n, args.steps, t, dfa.start, k, p, seed=r)
            t2 = time.perf_counter()
            assert len(toks) == args.steps
            ext.append((t1 - t0) * 1e3 / args.steps)
            con.append((t2 - t1) * 1e3 / args.steps)
        me, mc = statistics.median(ext), statistics.median(con)
        print(f"  loops, {label:<24}: extended {me:.4f} ms/step ({1e3 / me:.1f} tok/s)   constrained {mc:.4f} ms/step "
              f"({1e3 / mc:.1f} tok/s)   {(mc - me) * 1e3:+.1f} us/step ({100 * (mc - me) / me:+.2f} %)", flush=True)


def ext_loop_rounds(m, n, args, widths):
    """ms/step of `rounds` xh_decode_sample_ext calls per top-N width, the widths in turn within a
    round (width None: xh_set_top_logprobs is never called, for a library without it)."""
    t, k, p = PARAMS
    out = {w: [] for w in widths}
    for w in widths:  # every graph exists and is warm
        if w is not None:
            m.set_top_logprobs(w)
        m.decode_sample_ext(n, 8, t, k, p, seed=1)
    for r in range(args.rounds):
        for w in widths:
            if w is not None:
                m.set_top_logprobs(w)
                m.decode_sample_ext(n, 1, t, k, p, seed=1)  # 0 <-> positive captures anew: outside the timing
            t0 = time.perf_counter()
            toks = m.decode_sample_ext(n, args.steps, t, k, p, seed=r)
            out[w].append((time.perf_counter() - t0) * 1e3 / args.steps)
            assert len(toks) == args.steps
    return out


def top_logprobs_rows(m, c, n, args, prompt, st):
    for w in (1, 5, 32):
        m.set_top_logprobs(w)
        us = m.time_kernel(9, args.head_iters)
        print(f"  top-N row kernel alone, n_top {w:<2}: {us:8.2f} us", flush=True)
    loops = ext_loop_rounds(m, n, args, (0, 5, 32))
    base = statistics.median(loops[0])
    for w, v in loops.items():
        med = statistics.median(v)
        print(f"  extended loop, n_top {w:<2}: " + " ".join(f"{x:.4f}" for x in v) + f"   median {med:.4f} ms/step"
              + (f"   {(med - base) * 1e3:+.1f} us/step ({100 * (med - base) / base:+.2f} %)" if w else ""), flush=True)
    m.set_top_logprobs(0)
    toks = [1] + [(i * 7919 + 13) % c.vocab_size for i in range(args.score_tokens - 1)]
    rows = {"xh_perplexity": lambda: m.token_probs(toks, 0), "xh_score n_top 0": lambda: m.score(toks, 0, 0),
            "xh_score n_top 5": lambda: m.score(toks, 0, 5)}
    for fn in rows.values():  # buffers allocated, kernels loaded
        m.reset()
        fn()
    times = {k: [] for k in rows}
    for r in range(args.rounds):
        for label, fn in rows.items():
            m.reset()
            t0 = time.perf_counter()
            fn()
            times[label].append((time.perf_counter() - t0) * 1e3)
    ppl = statistics.median(times["xh_perplexity"])
    for label, v in times.items():
        med = statistics.median(v)
        print(f"  {label:<17} {args.score_tokens} tokens: " + " ".join(f"{x:.2f}" for x in v) + f"   median {med:.2f} ms"
              + (f"   {med - ppl:+.2f} ms ({100 * (med - ppl) / ppl:+.2f} %)" if label != "xh_perplexity" else ""), flush=True)
    m.reset()
    m.prefill(prompt, 0, st)


ADAPT_SETS = [("off", PARAMS, {}), ("n-sigma 1.0", PARAMS, dict(top_n_sigma=1.0)),
              ("typical 0.9", PARAMS, dict(typical_p=0.9)),
              ("Mirostat tau 5 eta 0.1", (0.8, 0, 1.0), dict(mirostat_tau=5.0, mirostat_eta=0.1))]


def adapt_rows(m, n, args):
    for label, (t, k, p), trunc in ADAPT_SETS:
        m.decode_sample_ext(n, 1, t, k, p, seed=3)
        ext_us = m.time_kernel(7, args.head_iters)
        m.decode_sample_adapt(n, 1, t, k, p, seed=3, **trunc)
        adp_us = m.time_kernel(10, args.head_iters)
        print(f"  heads alone, t {t} k {k} p {p}, {label:<22}: extended (7) {ext_us:8.2f} us   adaptive (10) {adp_us:8.2f} us"
              f"   ({adp_us - ext_us:+.2f} us)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--head-iters", type=int, default=200)
    ap.add_argument("--constrained", type=int, default=1, help="also time the constrained head and loop")
    ap.add_argument("--top-logprobs", type=int, default=0, help="also time the top-N row kernel, loop and xh_score")
    ap.add_argument("--only-top", type=int, default=0, help="with --top-logprobs: nothing else")
    ap.add_argument("--score-tokens", type=int, default=2048)
    ap.add_argument("--adapt", type=int, default=0, help="also time the adaptive head against the extended head")
    ap.add_argument("--only-adapt", type=int, default=0, help="with --adapt: nothing else")
    args = ap.parse_args()
    for name in ("mistral-7b-f16", "llama3-8b-f16"):
        w = bench.WORKLOADS[name]
        c = bench.make_config(w)
        m = Model(c)
        for kind, layer, tdt, seed, mean, std in bench.tensor_specs(w):
            m.upload_synthetic(kind, layer, tdt, seed, mean, std)
        st = InferenceState(c)
        prompt = bench.prompt_tokens(c.vocab_size)
        m.prefill(prompt, 0, st)
        n = len(prompt)
        if args.top_logprobs and args.only_top:
            print(f"{name} (V = {c.vocab_size}), {args.steps} steps per call")
            top_logprobs_rows(m, c, n, args, prompt, st)
            m.close()
            continue
        if args.adapt and args.only_adapt:
            print(f"{name} (V = {c.vocab_size}), {args.head_iters} launches per figure")
            adapt_rows(m, n, args)
            m.close()
            continue
        m.decode_greedy(n, 8)  # capture both graphs and warm up before timing
        m.decode_sample(n, 8, *PARAMS, seed=1)
        greedy, sampled = [], []
        for r in range(args.rounds):
            t0 = time.perf_counter()
            m.decode_greedy(n, args.steps)
            t1 = time.perf_counter()
            m.decode_sample(n, args.steps, *PARAMS, seed=r)
            t2 = time.perf_counter()
            greedy.append((t1 - t0) * 1e3 / args.steps)
            sampled.append((t2 - t1) * 1e3 / args.steps)
        print(f"{name} (V = {c.vocab_size}), {args.steps} steps per call, ms/step by round")
        print("  greedy : " + " ".join(f"{v:.4f}" for v in greedy) + f"   median {statistics.median(greedy):.4f}")
        print("  sampled: " + " ".join(f"{v:.4f}" for v in sampled) + f"   median {statistics.median(sampled):.4f}")
        d = statistics.median(sampled) - statistics.median(greedy)
        print(f"  sampled - greedy: {d * 1e3:+.1f} us/step ({100 * d / statistics.median(greedy):+.2f} %)")
        for label, (t, k, p) in HEAD_SETS:
            m.decode_sample(n, 1, t, k, p, seed=3)  # sets the parameter block
            us = m.time_kernel(6, args.head_iters)
            print(f"  sample head alone, {label:<18}: {us:8.2f} us", flush=True)
        t, k, p = PARAMS
        for label, hist, ctl in ext_sets(c.vocab_size):
            m.decode_sample_ext(n, 1, t, k, p, seed=3, history=hist, **ctl)  # sets the blocks and the ring
            us = m.time_kernel(7, args.head_iters)
            print(f"  extended head alone, t {t} k {k} p {p}, {label:<22}: {us:8.2f} us", flush=True)
        if args.constrained:
            m.prefill(prompt, 0, st)  # the timed heads moved the position: hydrate again
            constrained_rows(m, c, n, args)
        if args.top_logprobs:
            m.prefill(prompt, 0, st)
            top_logprobs_rows(m, c, n, args, prompt, st)
        if args.adapt:
            m.prefill(prompt, 0, st)
            adapt_rows(m, n, args)
        m.close()


if __name__ == "__main__":
    main()
