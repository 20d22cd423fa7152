#!/usr/bin/env python
"""Prompt passes past the wrap of a full fp8 (e4m3) KV ring: ring passes (XH_OPT_PREFILL_RING_KV8 1)
against the token loop (0, the only route before the option), next to the fp16 ring's ring passes.

Mistral-7B shapes with 8 layers, f16 weights, max_seq_len 32768, the rings full of synthetic K/V
(xh_kv_fill_synthetic), xh_prefill of N tokens at pos0 = max_seq_len + 1000.  One process per N holds
three contexts with the same weights: an fp16 ring, an fp8 ring with XH_OPT_PREFILL_ATTN_KV8 1 and
XH_OPT_PREFILL_RING_KV8 0, and an fp8 ring with both 1.  Every context is warmed by two untimed calls
(the first builds the pass buffers), then `--rounds` timed calls per context, the contexts in turn
within a round; the median is reported with the least and the greatest.  The host clock stands
around a call that ends with the logits on the host, so the device is drained.  Every call rewrites
the same ring slots from the same pos0, so its work does not depend on the calls before it.

The driver (no device of its own) starts one measuring process per N under its own `timeout`, with at
most 16 CPU threads, and starts nothing after a step that failed.

    python tools/kv8_ring_time.py > profiles/kv8_ring_time.txt
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("f16 ring", "f8 ring, RING_KV8 0", "f8 ring, RING_KV8 1")


def measure(args, n):
    sys.path.insert(0, ROOT)
    import bench
    from xalm_amd import _lib as L
    from xalm_amd.model import InferenceState, Model

    w = dict(bench.WORKLOADS["mistral-7b-f16-32k"], layers=args.layers)
    msl = w["msl"]
    pos0 = msl + 1000

    def build(kv_dtype, ring_kv8):
        m = Model(bench.make_config(w), 0, kv_dtype)
        for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
            m.upload_synthetic(kind, layer, dt, seed, mean, std)
        m.set_option(L.OPT_PREFILL_ATTN_KV8, 1)
        m.set_option(L.OPT_PREFILL_RING_KV8, ring_kv8)
        for layer in range(m.config.n_layers):
            m.kv_fill_synthetic(layer, 0, 0, msl, 5000 + 2 * layer, 1.0)
            m.kv_fill_synthetic(layer, 1, 0, msl, 5001 + 2 * layer, 1.0)
        return m

    ctx = dict(zip(NAMES, (build(L.F16, 0), build(L.F8_E4M3, 0), build(L.F8_E4M3, 1))))
    toks = bench.prompt_tokens(w["vocab"], n=n, seed=17)
    st = {k: InferenceState(m.config) for k, m in ctx.items()}
    for k, m in ctx.items():
        for _ in range(2):
            m.prefill(toks, pos0, st[k])
    sec = {k: [] for k in ctx}
    for _ in range(args.rounds):
        for k, m in ctx.items():
            t0 = time.perf_counter()
            m.prefill(toks, pos0, st[k])
            sec[k].append(time.perf_counter() - t0)
    ms = {}
    for k, m in ctx.items():
        ms[k] = 1e3 * statistics.median(sec[k])
        nb, npass = m.prefill_route(n, pos0)
        print(f"n {n:5d} at pos0 {pos0}: {k:>20} ({nb:4d} tokens in {npass} passes) {ms[k]:10.3f} ms"
              f"  [{1e3 * min(sec[k]):10.3f} .. {1e3 * max(sec[k]):10.3f}]", flush=True)
    f16, loop, ring = (ms[k] for k in NAMES)
    print(f"n {n:5d}: token loop / fp8 ring pass = {loop / ring:.2f}   fp16 ring pass / fp8 ring pass = {f16 / ring:.3f}",
          flush=True)
    for m in ctx.values():
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="*", default=[32, 256, 2048])
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds per measuring process")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        measure(args, args.child)
        return 0
    print(f"Mistral-7B shapes, {args.layers} layers, f16 weights, max_seq_len 32768, the rings full; xh_prefill at pos0 = "
          f"max_seq_len + 1000")
    print(f"fp8 contexts: XH_OPT_PREFILL_ATTN_KV8 1, XH_OPT_PREFILL_RING_KV8 (RING_KV8) 0 / 1; median of {args.rounds} calls "
          f"per context after 2 warm-ups, the contexts in turn [least .. greatest]", flush=True)
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
        env[var] = str(min(16, int(env.get(var) or 16)))
    for n in args.n:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(n),
               "--layers", str(args.layers), "--rounds", str(args.rounds)]
        rc = subprocess.call(cmd, env=env)
        if rc != 0:
            print(f"n {n}: the measuring process ended with status {rc}; nothing further is started", flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
