"""Generate the MXFP4 fixtures under tests/golden/.

* ``tiny_mistral_mxfp4.xalm``: ``tiny_mistral_f32.xalm`` through tools/xalm_requant.py
  ``--type mxfp4`` (every weight matrix re-quantized by xh_quantize_blocks, norms and tokenizer
  copied).  Before it is written the oracle alone checks, on the CPU, that the six greedy steps
  after the 9-token prompt of tests/mxfp4_ref.py ``loop_tokens`` leave at least five with a
  top-two gap above 1e-3 (what tests/test_mxfp4_gpu.py compares); if not, change LOOP_STRIDE there.
* ``mxfp4_golden.npz``: ``values`` float32 [blocks][32], ``bytes`` uint8 [blocks][17] and
  ``deq`` float32 [blocks][32], all from the numpy reference of tests/mxfp4_ref.py: random blocks
  over 40 octaves, every tie under three scales and both signs, saturation, zeros, f32
  subnormals, amax at exact powers of two.

Run from the repository root after `make`:  python tests/golden/make_mxfp4_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mxfp4_ref as R  # noqa: E402
import xalm_requant  # noqa: E402
from xalm_amd.xalm_file import XalmFile  # noqa: E402

TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


def golden_inputs():
    rng = np.random.default_rng(20250)
    rows = []
    # random blocks, each under its own magnitude over 40 octaves
    scale = np.exp2(rng.uniform(-20, 20, (256, 1)))
    rows.append((rng.standard_normal((256, 32)) * scale).astype(np.float32))
    # ties: the block's amax 6 * s fixes E, the other elements sit on the midpoints (both signs)
    for s in (1.0, 2.0 ** -9, 2.0 ** 30):
        for sign in (1.0, -1.0):
            b = np.zeros(32, np.float32)
            b[0] = 6.0 * s
            b[1:8] = np.array(TIES, np.float32) * s * sign
            b[8:15] = np.nextafter(np.array(TIES, np.float32) * np.float32(s), np.float32(np.inf)) * sign
            b[15:22] = np.nextafter(np.array(TIES, np.float32) * np.float32(s), np.float32(0)) * sign
            b[22] = -0.0
            rows.append(b[None])
    # saturation: amax just below a power of two, so amax * 2^-E is close to 8
    b = np.full(32, 7.9, np.float32)
    b[::3] = -7.99
    b[1] = 6.5
    b[2] = 4.0
    rows.append(b[None])
    rows.append(np.zeros((1, 32), np.float32))
    rows.append(np.full((1, 32), -0.0, np.float32))
    # f32 subnormals (E clamps at -127) and the smallest normals
    sub = (rng.integers(0, 1 << 23, (4, 32)).astype(np.uint32)).view(np.float32) * rng.choice([-1, 1], (4, 32)).astype(np.float32)
    rows.append(sub)
    tiny = np.zeros((1, 32), np.float32)
    tiny[0, :4] = np.array([1, 2, 3, 7], np.uint32).view(np.float32)
    rows.append(tiny)
    rows.append((rng.standard_normal((2, 32)) * 2.0 ** -125).astype(np.float32))
    # amax at exact powers of two, across the exponent range.  (Nothing below 2^-128: such a block
    # is all (+-)0 codes, and its values, all zero, quantize to the all-zero block, not to itself;
    # tests/test_mxfp4_cpu.py walks every power of two down to 2^-149 against the reference.)
    for p in (-128, -126, -30, -1, 0, 1, 17, 100, 127):
        b = (rng.uniform(-1, 1, 32) * 2.0 ** p).astype(np.float32)
        b[5] = np.float32(2.0 ** p)
        rows.append(b[None])
    rows.append((rng.standard_normal((4, 32)) * 2.0 ** 120).astype(np.float32))
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def main():
    v = golden_inputs()
    by = R.quantize(v)
    np.savez_compressed(os.path.join(HERE, "mxfp4_golden.npz"), values=v, bytes=by, deq=R.dequantize(by))
    print("mxfp4_golden.npz:", v.shape[0], "blocks")

    src = os.path.join(HERE, "tiny_mistral_f32.xalm")
    dst = os.path.join(HERE, "tiny_mistral_mxfp4.xalm")
    tmp = dst + ".tmp"
    n = xalm_requant.requant(src, tmp, "mxfp4")
    xf = XalmFile(tmp)
    om = R.oracle_from_xalm(xf)
    toks = R.loop_tokens(xf.config().vocab_size)
    clear = R.greedy_gap_count(om, toks)
    om.close()
    del xf
    assert clear >= 5, f"only {clear} of 6 greedy steps have a clear top-two gap: change mxfp4_ref.LOOP_STRIDE"
    os.replace(tmp, dst)
    print(f"tiny_mistral_mxfp4.xalm: {n} tensors, {os.path.getsize(dst)} bytes, {clear}/6 greedy steps clear")


if __name__ == "__main__":
    main()
