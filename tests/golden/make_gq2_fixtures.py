"""Generate the fixtures of the affine and 5-bit gguf blocks (Q4_1 / Q5_0 / Q5_1) under tests/golden/.

* ``tiny_mistral_q4_1.xalm``, ``tiny_mistral_q5_0.xalm``, ``tiny_mistral_q5_1.xalm``: the
  tiny_mistral checkpoint of make_fixtures.py, written by the REFERENCE converter (convert.py
  ``--type q4_1 / q5_0 / q5_1``: XType.convert_to -> quants.py ``quantize``), run in memory as
  make_fixtures.py does.
* ``gq2_golden.npz``: the input rows of make_gq_fixtures.py ``gq_inputs()`` plus a row of
  constant blocks (max == min, so d == 0) and an all-positive row (m > 0, d*q never cancels),
  with the bytes of quants.py ``quantize`` and the floats of quants.py ``dequantize`` for the
  three types.  They pin the shared quantizer (include/xalm_synth.h, xh_quantize_blocks) and
  the tests' numpy dequantizer (tests/gq2_ref.py) bit for bit.

Run:  python tests/golden/make_gq2_fixtures.py      (needs the reference checkout, torch)
"""
from __future__ import annotations

import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf  # noqa: E402
import make_gq_fixtures as mgq  # noqa: E402

TYPES = ("q4_1", "q5_0", "q5_1")


def gq2_inputs():
    rng = np.random.default_rng(2025)
    const = np.repeat(rng.normal(0.0, 0.5, 8).astype(np.float32), 32)   # 8 constant blocks: d == 0
    const[:32] = 0.0
    pos = rng.uniform(0.5, 1.5, 256).astype(np.float32)                 # all positive: m > 0
    return np.concatenate([mgq.gq_inputs(), np.stack([const, pos])])


def main():
    sys.path.insert(0, mf.REF)
    import quants  # the reference's quantizer (imported from the reference checkout, not copied)

    x = gq2_inputs()
    out = {"inputs": x}
    for name in TYPES:
        qt = getattr(quants.GGMLQuantizationType, name.upper())
        q = quants.quantize(x, qt)
        out[name] = np.ascontiguousarray(q, dtype=np.uint8)
        out[name + "_deq"] = np.ascontiguousarray(quants.dequantize(q, qt), dtype=np.float32)
    np.savez_compressed(os.path.join(HERE, "gq2_golden.npz"), **out)
    print("wrote gq2_golden.npz", {k: v.shape for k, v in out.items()})

    import torch  # noqa: F401
    conv = mf.load_reference_converter()
    spec = mf.MODELS["tiny_mistral"]
    tmp = tempfile.mkdtemp(prefix="xalm_gq2_tiny_mistral_")
    try:
        mf.write_checkpoint(tmp, spec)
        for t in TYPES:
            path = os.path.join(HERE, f"tiny_mistral_{t}.xalm")
            mf.convert(conv, tmp, path, t)
            print("wrote", path, os.path.getsize(path))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
