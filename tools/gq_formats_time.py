#!/usr/bin/env python
"""Decode launches of the five gguf block formats, timed side by side in one process.

For each of Q8_0, Q4_0, Q4_1, Q5_0, Q5_1: a context with Mistral-7B's shapes (8 layers, so the
rotating launches never find their weights in the Infinity Cache) and synthetic weights of that
one block dtype, then xh_time_kernel / xh_kernel_bytes for launches 0..4 (W1/W3, qkv, Wo, W2,
lm_head).  One GPU process, one context at a time; two rounds, so drift shows.  The comparison
is between formats inside one run on one box, never across boxes.

Run under a time limit:  timeout -k 10 600 python tools/gq_formats_time.py [--iters N]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from xalm_amd import _lib as L  # noqa: E402
from xalm_amd.model import InferenceState, Model  # noqa: E402

FORMATS = [("Q8_0", L.Q8_0), ("Q4_0", L.Q4_0), ("Q4_1", L.Q4_1), ("Q5_0", L.Q5_0), ("Q5_1", L.Q5_1)]
LAUNCHES = ["W1/W3", "qkv", "Wo", "W2", "lm_head"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=8)
    args = ap.parse_args()
    print(f"Mistral-7B shapes, {args.layers} layers, synthetic block weights; {args.iters} launches per figure")
    print(f"{'round':>5} {'format':>6} {'B/blk':>5} " + " ".join(f"{n + ' us':>10} {'TB/s':>6}" for n in LAUNCHES), flush=True)
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
            print(f"{rnd:>5} {name:>6} {L.GQ_BLOCK_BYTES[dt]:>5} " + " ".join(cells), flush=True)
            m.close()


if __name__ == "__main__":
    main()
