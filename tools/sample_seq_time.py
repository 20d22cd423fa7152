"""Device time of the sequence-aware step head (xh_time_kernel 11) next to the adaptive head (10) in the
same run, on bench.py's synthetic workloads: everything off, DRY + the n-gram ban over a full
1024-token window, and XTC firing on every launch.

    python tools/sample_seq_time.py [--head-iters 200] [--rounds 3]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from xalm_amd.model import InferenceState, Model  # noqa: E402

PARAMS = (0.8, 40, 0.95)


def seq_sets(vocab):
    # a window of period 97: every launch finds about ten earlier occurrences of its last token, each
    # matched back to the 64-token cap, and one follower to penalise and ban
    hist = [(7 + 13 * (i % 97)) % vocab for i in range(1024)]
    return [("everything off", [], {}),
            ("DRY + n-gram 3, window 1024", hist, dict(dry_multiplier=0.8, dry_base=1.75, dry_allowed_length=2,
                                                       no_repeat_ngram=3, seq_last_n=1024, breakers=range(0, 2048, 2))),
            ("XTC p 1.0 thr 0.1", [], dict(xtc_probability=1.0, xtc_threshold=0.1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head-iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    t, k, p = PARAMS
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
        print(f"{name} (V = {c.vocab_size}), t {t} k {k} p {p}, {args.head_iters} launches per figure, median of {args.rounds}")
        for label, hist, seq in seq_sets(c.vocab_size):
            adp, sq = [], []
            for _ in range(args.rounds):
                m.decode_sample_adapt(n, 1, t, k, p, seed=3, history=hist)
                adp.append(m.time_kernel(10, args.head_iters))
                m.decode_sample_seq(n, 1, t, k, p, seed=3, history=hist, **seq)
                sq.append(m.time_kernel(11, args.head_iters))
            a, s = statistics.median(adp), statistics.median(sq)
            print(f"  {label:<28}: adaptive (10) {a:8.2f} us   sequence (11) {s:8.2f} us   ({s - a:+.2f} us, "
                  f"{100 * (s - a) / a:+.2f} %)", flush=True)
        m.close()


if __name__ == "__main__":
    main()
