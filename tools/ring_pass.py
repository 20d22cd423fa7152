#!/usr/bin/env python
"""Prompt passes past the KV ring wrap, ring passes (XH_OPT_PREFILL_RING 1) against the token loop (0).

* mistral-7b-f16-32k (configs[3] shapes, synthetic weights, the rings full of synthetic K/V):
  xh_prefill of N tokens at pos0 = max_seq_len + 1000, REPEAT times each way.  The yardstick just
  before the wrap is tools/short_pass.py (the same N at pos0 = max_seq_len - N).
* mistral-7b-f16 (-T 4096): token_probs over 8193 tokens from pos 0, each way (--no-ppl skips it).
For rocprofv3 kernel stats of one ring pass:
    rocprofv3 --kernel-trace --stats -d OUT -- python3 tools/ring_pass.py 32 --ring 1 --no-ppl
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from xalm_amd import _lib as L  # noqa: E402
from xalm_amd.model import InferenceState, Model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n", type=int, nargs="*", default=[2, 8, 32, 256, 2048])
ap.add_argument("--ring", type=int, nargs="+", default=[1, 0])
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--no-ppl", action="store_true")
ap.add_argument("--ppl-tokens", type=int, default=8193)
args = ap.parse_args()


def build(name):
    w = bench.WORKLOADS[name]
    c = bench.make_config(w)
    m = Model(c)
    for kind, layer, dt, seed, mean, std in bench.tensor_specs(w):
        m.upload_synthetic(kind, layer, dt, seed, mean, std)
    return c, m


if args.n:
    c, m = build("mistral-7b-f16-32k")
    for layer in range(c.n_layers):
        m.kv_fill_synthetic(layer, 0, 0, c.max_seq_len, 5000 + 2 * layer, 1.0)
        m.kv_fill_synthetic(layer, 1, 0, c.max_seq_len, 5001 + 2 * layer, 1.0)
    st = InferenceState(c)
    pos0 = c.max_seq_len + 1000
    for n in args.n:
        toks = bench.prompt_tokens(c.vocab_size, n=n, seed=17)
        for ring in args.ring:
            m.set_option(L.OPT_PREFILL_RING, ring)
            nb, npass = m.prefill_route(n, pos0)
            ts = []
            for _ in range(args.repeat + 1):  # the first run warms buffers and code objects
                t0 = time.perf_counter()
                m.prefill(toks, pos0, st)
                ts.append(1e3 * (time.perf_counter() - t0))
            print(f"32k n {n} ring {ring} ({nb} tokens in {npass} passes): warm-up {ts[0]:.3f} ms, then "
                  f"{' '.join(f'{t:.3f}' for t in ts[1:])}", flush=True)
    m.close()

if not args.no_ppl:
    c, m = build("mistral-7b-f16")
    toks = bench.prompt_tokens(c.vocab_size, n=args.ppl_tokens, seed=19)
    for ring in args.ring:
        m.set_option(L.OPT_PREFILL_RING, ring)
        nb, npass = m.prefill_route(len(toks) - 1, 0)
        ts = []
        for _ in range(2):
            m.reset()
            t0 = time.perf_counter()
            m.token_probs(toks)
            ts.append(time.perf_counter() - t0)
        print(f"4k token_probs {len(toks)} tokens ring {ring} ({nb} tokens in {npass} passes): warm-up "
              f"{ts[0]:.3f} s, then {ts[1]:.3f} s = {(len(toks) - 1) / ts[1]:.1f} tok/s", flush=True)
    m.close()
