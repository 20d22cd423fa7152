#!/usr/bin/env python
"""Sampled against greedy decode on the device, timed side by side in one process.

For the synthetic Mistral-7B f16 (V = 32000) and Llama-3-8B f16 (V = 128256) shapes: a 32-token
prompt, then 128-step xh_decode_greedy and xh_decode_sample (temperature 0.8, top_k 40, top_p
0.95) calls in turn, six of each, every call from the same position; ms/step of both and their
difference.  Then the sampled step head's own device time (xh_time_kernel 6, HIP events) under
three parameter sets, and the extended step head's (xh_time_kernel 7, xh_decode_sample_ext) at the
first of them with its controls off, with a 64-token window, and with a 1024-token window and 256
biases.  The comparison is the greedy loop of the same process on the same box.

Run under a time limit:  timeout -k 10 600 python tools/sample_time.py
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--head-iters", type=int, default=200)
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
        m.close()


if __name__ == "__main__":
    main()
