#!/usr/bin/env python
"""The K-quants Q4_K / Q6_K beside Q4_0 / Q4_1 / Q8_0, timed side by side in one process.

Contexts with Mistral-7B's shapes (8 layers, so the rotating launches never find their weights in
the Infinity Cache) and synthetic weights of one block dtype, the five formats alternating for two
rounds: xh_time_kernel / xh_kernel_bytes for launches 0..4 (W1/W3, qkv, Wo, W2, lm_head), a
256-step decode_greedy in tok/s and a 2048-token prefill in tok/s (each run twice, the second
timed: the first allocates buffers and captures the decode graph).  The yardsticks are Q4_1 (for Q4_K: the same
arithmetic at 20 bytes per 32 elements against 18) and Q8_0 (for Q6_K: 34 bytes against 26.25) in the
same run on the same box; the margin is the spread between the run's own two rounds.

The table goes to stdout and to profiles/kq_time.txt (--out).

Run under a time limit:  timeout -k 10 900 python tools/kq_time.py [--iters N]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from xalm_amd import _lib as L  # noqa: E402
from xalm_amd.model import InferenceState, Model  # noqa: E402

FORMATS = [("Q4_0", L.Q4_0), ("Q4_1", L.Q4_1), ("Q4_K", L.Q4_K), ("Q6_K", L.Q6_K), ("Q8_0", L.Q8_0)]
LAUNCHES = ["W1/W3", "qkv", "Wo", "W2", "lm_head"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--prompt", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kq_time.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(a_out := args.out) or ".", exist_ok=True)
    log = open(a_out, "w")

    def print(line, flush=True):  # noqa: A001 - every line to stdout and to the file
        sys.stdout.write(line + "\n")
        sys.stdout.flush()
        log.write(line + "\n")
        log.flush()

    print(f"Mistral-7B shapes, {args.layers} layers, synthetic block weights; {args.iters} launches per figure, "
          f"{args.steps}-step greedy decode, {args.prompt}-token prefill")
    print(f"{'round':>5} {'format':>6} {'B/32':>6} " + " ".join(f"{n + ' us':>10} {'TB/s':>6}" for n in LAUNCHES) +
          f" {'decode tok/s':>13} {'prefill tok/s':>14}", flush=True)
    for rnd in range(args.rounds):
        for name, dt in FORMATS:
            w = dict(bench.WORKLOADS["mistral-7b-f16"], layers=args.layers, wdt=dt, edt=dt, cdt=dt)
            c = bench.make_config(w)
            m = Model(c)
            for kind, layer, tdt, seed, mean, std in bench.tensor_specs(w):
                m.upload_synthetic(kind, layer, tdt, seed, mean, std)
            st = InferenceState(c)
            m.forward(st, 1, 0)
            cells = []
            for which in range(5):
                us = m.time_kernel(which, args.iters)
                cells.append(f"{us:10.2f} {m.kernel_bytes(which, 1) / us * 1e-6:6.2f}")
            toks = [1] + [3 + (i * 41) % (c.vocab_size - 3) for i in range(args.prompt - 1)]
            dec = pre = 0.0
            for _ in range(2):
                m.reset()
                m.prefill(toks[:32], 0, st)
                t0 = time.perf_counter()
                out = m.decode_greedy(32, args.steps)
                dec = len(out) / (time.perf_counter() - t0)
            for _ in range(2):
                m.reset()
                t0 = time.perf_counter()
                m.prefill(toks, 0, st)
                pre = len(toks) / (time.perf_counter() - t0)
            print(f"{rnd:>5} {name:>6} {L.row_bytes(dt, 256) / 8:>6.2f} " + " ".join(cells) + f" {dec:13.1f} {pre:14.1f}", flush=True)
            m.close()


if __name__ == "__main__":
    main()
