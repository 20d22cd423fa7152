#!/usr/bin/env python
"""The fp8 (e4m3) KV ring next to the fp16 ring, timed in one process.

Mistral-7B shapes with 8 layers, f16 weights, max_seq_len 32768.  One fp16-KV context and one
fp8-KV context hold the same synthetic weights.  At a history of 4096 and of 32768 slots (the
rings filled with xh_kv_fill_synthetic, one forward at the last position): the attention launch
alone (xh_time_kernel 5, HIP events, launches rotating over the layers) and the device greedy
loop's tok/s (128-step calls from the same position, the median of 5, the two contexts in turn).
Then the rate of a 2048-token xh_prefill from a reset context.  The fp16 figure stands beside
every fp8 one; the ratios are fp8 / fp16.

An fp8 context decodes every layer on the two-launch route (attention, then Wo) and runs the
prompt attention as under XH_OPT_PREFILL_ATTN 0; the fp16 context keeps its defaults (the fused
attention + Wo launch, the MFMA prompt attention), so the loop and prefill rows carry that cost.

Run under a time limit:  timeout -k 10 600 python tools/kv8_time.py > profiles/kv8_time.txt
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


def build(w, kv_dtype):
    m = Model(bench.make_config(w), 0, kv_dtype)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
        m.upload_synthetic(kind, layer, dt, seed, mean, std)
    return m


def at_history(m, hist):
    """Rings full up to `hist` slots, the step parameters at the last of them."""
    m.reset()
    for layer in range(m.config.n_layers):
        m.kv_fill_synthetic(layer, 0, 0, hist - 1, 5000 + 2 * layer, 1.0)
        m.kv_fill_synthetic(layer, 1, 0, hist - 1, 5001 + 2 * layer, 1.0)
    m.forward(InferenceState(m.config), 17, hist - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    w = dict(bench.WORKLOADS["mistral-7b-f16-32k"], layers=args.layers)
    ctx = {"f16": build(w, L.F16), "f8": build(w, L.F8_E4M3)}
    kv_dim = w["kv_heads"] * w["head_dim"]
    print(f"Mistral-7B shapes, {args.layers} layers, f16 weights, max_seq_len {w['msl']}; KV ring f16 | f8 (e4m3)")
    for hist in (4096, 32768):
        for m in ctx.values():
            at_history(m, hist)
        us = {k: m.time_kernel(5, args.iters) for k, m in ctx.items()}
        gb = {k: m.kernel_bytes(5, hist) / 1e9 for k, m in ctx.items()}
        print(f"kv_len {hist:5d}  attention launch (xh_time_kernel 5): f16 {us['f16']:8.2f} us ({gb['f16'] / us['f16'] * 1e6:6.0f} GB/s)"
              f"   f8 {us['f8']:8.2f} us ({gb['f8'] / us['f8'] * 1e6:6.0f} GB/s)   f8 / f16 = {us['f8'] / us['f16']:.3f}", flush=True)
        for m in ctx.values():
            m.decode_greedy(hist, 8)  # the graph exists and is warm
        ms = {k: [] for k in ctx}
        for _ in range(args.rounds):
            for k, m in ctx.items():
                t0 = time.perf_counter()
                assert len(m.decode_greedy(hist, args.steps)) == args.steps
                ms[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(f"kv_len {hist:5d}  greedy loop, {args.steps} steps x {args.rounds}: f16 {1e3 / med['f16']:8.1f} tok/s"
              f"   f8 {1e3 / med['f8']:8.1f} tok/s   f8 / f16 = {med['f16'] / med['f8']:.3f}"
              f"   (KV bytes per step: {2 * args.layers * hist * kv_dim * 2 / 1e6:.0f} | {2 * args.layers * hist * kv_dim / 1e6:.0f} MB)",
              flush=True)
    toks = bench.prompt_tokens(w["vocab"], 2048)
    rate = {}
    for k, m in ctx.items():
        best = None
        for _ in range(3):  # the first builds the pass buffers
            m.reset()
            t0 = time.perf_counter()
            m.prefill(toks, 0, InferenceState(m.config))
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        rate[k] = len(toks) / best
        print(f"prefill 2048 tokens, route {m.prefill_route(len(toks), 0)}: KV {k:>3} {rate[k]:9.0f} tok/s", flush=True)
    print(f"prefill f8 / f16 = {rate['f8'] / rate['f16']:.3f}")


if __name__ == "__main__":
    main()
