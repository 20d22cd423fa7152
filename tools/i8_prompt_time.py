#!/usr/bin/env python
"""The prompt passes over the 32-element gguf block weights under XH_OPT_PREFILL_I8 (the int8 MFMA GEMM against
activations quantised per block, gemm_i8.h), next to XH_OPT_PREFILL_GQ (the f16 block-code GEMM, gemm_gq.h), to
neither option, and to f16 weights, timed in one process.

Mistral-7B shapes with 8 layers, synthetic weights, max_seq_len 4096.  Five weight sets (Q8_0, Q4_0, Q4_1,
Q5_0, Q5_1 everywhere), each as "opt 0" (Q8_0 / Q4_0 / Q5_0: gemm16.h over hi + lo f16 images; Q4_1 / Q5_1: the
f32-input MFMA kernel in 64-token passes), "GQ 1" and "I8 1" (the quantiser's launches included: it runs once per
GEMM input inside the pass), and f16 weights (gemm16.h as stored).  Three figures, all xh_prefill at pos0 0 from a
reset context: (a) 2048 tokens, (b) 256 tokens, (c) 32 tokens (GEMMs over at most 64 tokens never take either route).

Each figure: every context warmed by two untimed calls (the first builds the pass buffers), then
`--rounds` timed calls per context, the contexts in turn within a round, the median reported with
the least and the greatest and the spread (greatest - least) / median.  The host clock stands around
a call that ends with the logits on the host, so the device is drained.  The other contexts run between
two calls of one, so no repeat finds its weights in the 256 MiB Infinity Cache.

Run under a time limit:  timeout -k 10 900 python tools/i8_prompt_time.py > profiles/i8_prompt_time.txt
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

FORMATS = [("Q8_0", L.Q8_0), ("Q4_0", L.Q4_0), ("Q4_1", L.Q4_1), ("Q5_0", L.Q5_0), ("Q5_1", L.Q5_1)]


def build(w, wdt, option=None):
    w = dict(w, wdt=wdt, edt=wdt, cdt=wdt)
    m = Model(bench.make_config(w), 0)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
        m.upload_synthetic(kind, layer, dt, seed, mean, std)
    if option is not None:
        m.set_option(option, 1)
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
    ap.add_argument("--prompts", type=int, nargs="+", default=[2048, 256, 32])
    ap.add_argument("--formats", nargs="+", default=[n for n, _ in FORMATS])
    args = ap.parse_args()
    w = dict(bench.WORKLOADS["mistral-7b-f16"], layers=args.layers)
    sets = [(n, dt) for n, dt in FORMATS if n in args.formats]
    ctx = {}
    for name, dt in sets:
        ctx[f"{name}, opt 0"] = build(w, dt)
        ctx[f"{name}, GQ 1"] = build(w, dt, L.OPT_PREFILL_GQ)
        ctx[f"{name}, I8 1"] = build(w, dt, L.OPT_PREFILL_I8)
    ctx["f16"] = build(w, L.F16)
    print(f"Mistral-7B shapes, {args.layers} layers, max_seq_len {w['msl']}; XH_OPT_PREFILL_I8 (I8) and XH_OPT_PREFILL_GQ (GQ) on gguf block weights, beside f16 weights")
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
            print(f"({tag}) prefill {n} tokens at pos0 0, route {m.prefill_route(n, 0)}: {k:>10} {ms[k]:9.3f} ms = {n / ms[k] * 1e3:9.0f} tok/s"
                  f"  [{min(sec[k]) * 1e3:9.3f} .. {max(sec[k]) * 1e3:9.3f}]  spread {(max(sec[k]) - min(sec[k])) * 1e3 / ms[k] * 100:.1f} %",
                  flush=True)
        for name, _dt in sets:
            i8, gq, o0 = ms[name + ", I8 1"], ms[name + ", GQ 1"], ms[name + ", opt 0"]
            print(f"({tag}) {name}: time I8 1 / GQ 1 = {i8 / gq:.3f}   I8 1 / opt 0 = {i8 / o0:.3f}   I8 1 / f16 = {i8 / ms['f16']:.3f}",
                  flush=True)


if __name__ == "__main__":
    main()
