#!/usr/bin/env python
"""The prompt passes over K-quant weights with and without XH_OPT_PREFILL_KQ, next to Q4_0 weights,
timed in one process.

Mistral-7B shapes with 8 layers, synthetic weights, max_seq_len 4096.  Three weight sets (Q4_K everywhere,
Q6_K everywhere, and the q4_k_m mix: Q4_K with Q6_K for embed, output and every mlp.down), each with the
option 0 (the f32-input MFMA kernel in 64-token passes: the path before the option, and the yardstick) and
1 (gemm_kq.h, one pass of up to 2048 tokens), and Q4_0 weights (gemm16.h through their f16 images).  Two
figures, both xh_prefill at pos0 0 from a reset context: (a) 2048 tokens, (b) 32 tokens.

Each figure: every context warmed by two untimed calls (the first builds the pass buffers), then
`--rounds` timed calls per context, the contexts in turn within a round, the median reported with
the least and the greatest and the spread (greatest - least) / median.  The host clock stands around
a call that ends with the logits on the host, so the device is drained.  The other contexts run between
two calls of one, so no repeat finds its weights in the 256 MiB Infinity Cache.

Run under a time limit:  timeout -k 10 600 python tools/kq_prompt_time.py > profiles/kq_prompt_time.txt
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from xalm_amd import _lib as L  # noqa: E402
from xalm_amd.model import InferenceState, Model  # noqa: E402

MIX_Q6 = (L.EMBED, L.WCLS, L.W2)  # q4_k_m's Q6_K tensors


def build(w, wdt, option, mix=False):
    w = dict(w, wdt=wdt, edt=wdt, cdt=wdt)
    m = Model(bench.make_config(w), 0)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
        if mix and dt == wdt and kind in MIX_Q6:
            dt = L.Q6_K
        m.upload_synthetic(kind, layer, dt, seed, mean, std)
    m.set_option(L.OPT_PREFILL_KQ, option)
    return m


def timed(ctx, call, rounds, warm=2):
    """seconds per call: {name: [rounds]}, the contexts in turn within a round"""
    for m in ctx.values():
        for _ in range(warm):
            call(m)
    out = {k: [] for k in ctx}
    for _ in range(rounds):
        for k, m in ctx.items():
            t0 = time.perf_counter()
            call(m)
            out[k].append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--prompts", type=int, nargs="+", default=[2048, 32])
    args = ap.parse_args()
    w = dict(bench.WORKLOADS["mistral-7b-f16"], layers=args.layers)
    sets = [("Q4_K", L.Q4_K, False), ("Q6_K", L.Q6_K, False), ("q4_k_m", L.Q4_K, True)]
    ctx = {}
    for name, dt, mix in sets:
        for option in (0, 1):
            ctx[f"{name}, KQ {option}"] = build(w, dt, option, mix)
    ctx["Q4_0"] = build(w, L.Q4_0, 0)
    print(f"Mistral-7B shapes, {args.layers} layers, max_seq_len {w['msl']}; XH_OPT_PREFILL_KQ (KQ) on K-quant weights, beside Q4_0 weights")
    print(f"median of {args.rounds} calls per context after 2 warm-ups, the contexts in turn [least .. greatest]")
    for tag, n in zip("abcdefgh", args.prompts):
        toks = bench.prompt_tokens(w["vocab"], n)

        def prompt(m):
            m.reset()
            m.prefill(toks, 0, InferenceState(m.config))

        sec = timed(ctx, prompt, args.rounds)
        ms = {}
        for k, m in ctx.items():
            ms[k] = statistics.median(sec[k]) * 1e3
            print(f"({tag}) prefill {n} tokens at pos0 0, route {m.prefill_route(n, 0)}: {k:>12} {ms[k]:9.3f} ms = {n / ms[k] * 1e3:9.0f} tok/s"
                  f"  [{min(sec[k]) * 1e3:9.3f} .. {max(sec[k]) * 1e3:9.3f}]  spread {(max(sec[k]) - min(sec[k])) * 1e3 / ms[k] * 100:.1f} %",
                  flush=True)
        for name, _dt, _mix in sets:
            print(f"({tag}) {name}: time KQ 1 / KQ 0 = {ms[name + ', KQ 1'] / ms[name + ', KQ 0']:.3f}   KQ 1 / Q4_0 = "
                  f"{ms[name + ', KQ 1'] / ms['Q4_0']:.3f}", flush=True)


if __name__ == "__main__":
    main()
