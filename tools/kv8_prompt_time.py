#!/usr/bin/env python
"""The prompt passes over an fp8 (e4m3) KV ring with and without XH_OPT_PREFILL_ATTN_KV8, next to
the fp16 ring, timed in one process.

Mistral-7B shapes with 8 layers, f16 weights, max_seq_len 32768.  Three contexts hold the same
synthetic weights: an fp16 ring, an fp8 ring with the option 0 (the prompt attention forced to the
per-token split kernel) and an fp8 ring with the option 1 (the MFMA kernels' fp8 form).  Two figures:

  (a) a 2048-token xh_prefill at pos0 0 from a reset context, in tok/s;
  (b) a 32-token xh_prefill at pos0 30000 over a synthetic history (xh_kv_fill_synthetic), in ms:
      one short pass whose attention walks 30000 slots per layer, where the history bytes dominate.

Each figure: every context warmed by two untimed calls (the first builds the pass buffers), then
`--rounds` timed calls per context, the contexts in turn within a round, the median reported with
the least and the greatest.  The host clock stands around a call that ends with the logits on the
host, so the device is drained.  A call walks all 8 layers (3.5 GB of weights; in (b) 0.98 GB of
fp16 or 0.49 GB of fp8 K/V), and the other contexts run between two calls of one, so no repeat finds
its rows in the 256 MiB Infinity Cache.  The fp16-ring and option-0 lines are the yardsticks of the
same run; ratios are against them.

Run under a time limit:  timeout -k 10 600 python tools/kv8_prompt_time.py > profiles/kv8_prompt_time.txt
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


def build(w, kv_dtype, option):
    m = Model(bench.make_config(w), 0, kv_dtype)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
        m.upload_synthetic(kind, layer, dt, seed, mean, std)
    m.set_option(L.OPT_PREFILL_ATTN_KV8, option)
    return m


def fill_history(m, hist):
    m.reset()
    for layer in range(m.config.n_layers):
        m.kv_fill_synthetic(layer, 0, 0, hist, 5000 + 2 * layer, 1.0)
        m.kv_fill_synthetic(layer, 1, 0, hist, 5001 + 2 * layer, 1.0)


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
    ap.add_argument("--prompt", type=int, default=2048)
    ap.add_argument("--hist", type=int, default=30000)
    ap.add_argument("--short", type=int, default=32)
    args = ap.parse_args()
    w = dict(bench.WORKLOADS["mistral-7b-f16-32k"], layers=args.layers)
    ctx = {"f16 ring": build(w, L.F16, 0), "f8 ring, KV8 0": build(w, L.F8_E4M3, 0), "f8 ring, KV8 1": build(w, L.F8_E4M3, 1)}
    print(f"Mistral-7B shapes, {args.layers} layers, f16 weights, max_seq_len {w['msl']}; XH_OPT_PREFILL_ATTN_KV8 (KV8) on the f8 (e4m3) ring")
    print(f"median of {args.rounds} calls per context, the contexts in turn [least .. greatest]")

    toks = bench.prompt_tokens(w["vocab"], args.prompt)

    def long_prompt(m):
        m.reset()
        m.prefill(toks, 0, InferenceState(m.config))

    sec = timed(ctx, long_prompt, args.rounds)
    rate = {}
    for k, m in ctx.items():
        rate[k] = args.prompt / statistics.median(sec[k])
        print(f"(a) prefill {args.prompt} tokens at pos0 0, route {m.prefill_route(args.prompt, 0)}: {k:>14} {rate[k]:9.0f} tok/s"
              f"  [{args.prompt / max(sec[k]):9.0f} .. {args.prompt / min(sec[k]):9.0f}]", flush=True)
    print(f"(a) KV8 1 / KV8 0 = {rate['f8 ring, KV8 1'] / rate['f8 ring, KV8 0']:.3f}   KV8 1 / f16 ring = {rate['f8 ring, KV8 1'] / rate['f16 ring']:.3f}"
          f"   KV8 0 / f16 ring = {rate['f8 ring, KV8 0'] / rate['f16 ring']:.3f}", flush=True)

    short = bench.prompt_tokens(w["vocab"], args.short, seed=11)
    for m in ctx.values():
        fill_history(m, args.hist)

    def short_pass(m):
        m.prefill(short, args.hist, InferenceState(m.config))

    sec = timed(ctx, short_pass, args.rounds)
    ms = {}
    kv_dim = w["kv_heads"] * w["head_dim"]
    for k, m in ctx.items():
        ms[k] = statistics.median(sec[k]) * 1e3
        esz = 2 if k.startswith("f16") else 1
        print(f"(b) prefill {args.short} tokens at pos0 {args.hist}, route {m.prefill_route(args.short, args.hist)}: {k:>14} {ms[k]:8.3f} ms"
              f"  [{min(sec[k]) * 1e3:8.3f} .. {max(sec[k]) * 1e3:8.3f}]   (history K/V: {2 * args.layers * args.hist * kv_dim * esz / 1e6:.0f} MB)",
              flush=True)
    print(f"(b) KV8 1 / KV8 0 = {ms['f8 ring, KV8 1'] / ms['f8 ring, KV8 0']:.3f}   KV8 1 / f16 ring = {ms['f8 ring, KV8 1'] / ms['f16 ring']:.3f}"
          f"   KV8 0 / f16 ring = {ms['f8 ring, KV8 0'] / ms['f16 ring']:.3f}")


if __name__ == "__main__":
    main()
