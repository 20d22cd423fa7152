#!/usr/bin/env python
"""Short prompt passes over the gguf block weights and the K-quants with and without XH_OPT_PREFILL_SHORT, next
to f16 weights, timed in one process.

Mistral-7B shapes with 8 layers, synthetic weights, max_seq_len 4096.  Seven weight sets (Q8_0, Q4_0, Q4_1,
Q5_0, Q5_1, Q4_K, Q6_K everywhere), each with the option 0 (GEMMs over at most 64 tokens on gemm16.h over hi + lo
f16 images rebuilt per matrix and pass for Q8_0 / Q4_0 / Q5_0, on the f32-input MFMA kernel for the others: the
path before the option, and the yardstick) and 1 (gemm_sk.h), and f16 weights (gemm16.h as stored).  Every
context has the long routes on (XH_OPT_PREFILL_GQ 1, XH_OPT_PREFILL_KQ 1), so only the short GEMMs differ.
Figures, all xh_prefill at pos0 0 from a reset context: 8, 32 and 64 tokens, and 2048 + 32 (a long pass with a
short tail).

Each figure: every context warmed by two untimed calls (the first builds the pass buffers), then
`--rounds` timed calls per context, the contexts in turn within a round, the median reported with
the least and the greatest and the spread (greatest - least) / median.  The host clock stands around
a call that ends with the logits on the host, so the device is drained.  The other contexts run between
two calls of one, so no repeat finds its weights in the 256 MiB Infinity Cache.

Run under a time limit:  timeout -k 10 900 python tools/sk_prompt_time.py > profiles/sk_prompt_time.txt
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

FORMATS = [("Q8_0", L.Q8_0), ("Q4_0", L.Q4_0), ("Q4_1", L.Q4_1), ("Q5_0", L.Q5_0), ("Q5_1", L.Q5_1), ("Q4_K", L.Q4_K),
           ("Q6_K", L.Q6_K)]


def build(w, wdt, option):
    w = dict(w, wdt=wdt, edt=wdt, cdt=wdt)
    m = Model(bench.make_config(w), 0)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
        m.upload_synthetic(kind, layer, dt, seed, mean, std)
    m.set_option(L.OPT_PREFILL_GQ, 1)
    m.set_option(L.OPT_PREFILL_KQ, 1)
    m.set_option(L.OPT_PREFILL_SHORT, option)
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
    ap.add_argument("--prompts", type=int, nargs="+", default=[8, 32, 64, 2048 + 32])
    ap.add_argument("--formats", nargs="+", default=[n for n, _ in FORMATS])
    args = ap.parse_args()
    w = dict(bench.WORKLOADS["mistral-7b-f16"], layers=args.layers)
    sets = [(n, dt) for n, dt in FORMATS if n in args.formats]
    ctx = {}
    for name, dt in sets:
        for option in (0, 1):
            ctx[f"{name}, SHORT {option}"] = build(w, dt, option)
    ctx["f16"] = build(w, L.F16, 0)
    print(f"Mistral-7B shapes, {args.layers} layers, max_seq_len {w['msl']}; XH_OPT_PREFILL_SHORT (SHORT) on gguf block and K-quant "
          "weights under XH_OPT_PREFILL_GQ 1 and XH_OPT_PREFILL_KQ 1, beside f16 weights")
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
            print(f"({tag}) prefill {n} tokens at pos0 0, route {m.prefill_route(n, 0)}: {k:>14} {ms[k]:9.3f} ms = {n / ms[k] * 1e3:9.0f} tok/s"
                  f"  [{min(sec[k]) * 1e3:9.3f} .. {max(sec[k]) * 1e3:9.3f}]  spread {(max(sec[k]) - min(sec[k])) * 1e3 / ms[k] * 100:.1f} %",
                  flush=True)
        for name, _dt in sets:
            print(f"({tag}) {name}: time SHORT 1 / SHORT 0 = {ms[name + ', SHORT 1'] / ms[name + ', SHORT 0']:.3f}   SHORT 1 / f16 = "
                  f"{ms[name + ', SHORT 1'] / ms['f16']:.3f}", flush=True)


if __name__ == "__main__":
    main()
