"""Generate the K-quant (Q4_K / Q6_K) fixtures under tests/golden/.

* ``small_llama_q4_k_m.md5``: the md5 of ``small_llama_f16.xalm`` through tools/xalm_requant.py
  ``--type q4_k_m`` (dims 512 / 512, head_dim 128: every row is two super-blocks).  The file itself
  (1.9 MB) is above the 1 MiB a committed file may have in this project, so the tests make it afresh in a temporary
  directory (a fraction of a second) and hold it to this digest.
* ``kq_golden.npz``, per format ``q4_k`` / ``q6_k``:
    ``<fmt>_values``  float32 [rows][256 k]  input rows (N(0, 1) over several octaves, a constant, an
                      all-positive row, a row with one 1e4 outlier, sub-blocks 2^10 apart, zeros)
    ``<fmt>_bytes``   uint8   the project quantizer's bytes for them (xh_quantize_blocks)
    ``<fmt>_random``  uint8   rows of random bytes, the f16 scale fields forced finite
    ``<fmt>_bytes_deq`` / ``<fmt>_random_deq``  float32  what the reference's quants.py
                      ``dequantize`` returns for the two byte sets
  quants.py is imported from the reference checkout when this script runs and is never copied.

* ``kq_unchanged.npz`` (``--unchanged``, needs a GPU): the logits of 8 forward steps on
  ``tiny_mistral_q4_0 / q4_1 / mxfp4.xalm``, recorded ONCE from a build of the commit before the
  K-quants (``XALM_HIP_LIB=<that build's libxalm_hip.so> python tests/golden/make_kq_fixtures.py
  --unchanged``): what tests/test_kq_gpu.py holds the untouched formats to, bit for bit.  Do not
  regenerate it from a later build.

Run from the repository root after `make`:  python tests/golden/make_kq_fixtures.py
(needs the reference checkout; ``XALM_REF`` or make_fixtures.REF names it)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kq_ref as R  # noqa: E402
import make_fixtures as mf  # noqa: E402
import xalm_requant  # noqa: E402
from xalm_amd import _lib as L  # noqa: E402

NAMES = {R.Q4_K: "q4_k", R.Q6_K: "q6_k"}


def golden_inputs() -> np.ndarray:
    rng = np.random.default_rng(2627)
    rows = [rng.standard_normal((8, 512)) * np.exp2(rng.integers(-10, 6, (8, 1)))]
    rows.append(np.full((1, 512), 0.37))
    rows.append(np.abs(rng.standard_normal((1, 512))) + 0.5)
    out = rng.standard_normal((1, 512))
    out[0, 77] = 1e4
    rows.append(out)
    step = rng.standard_normal((1, 512))
    step[0, 32:64] *= 2.0 ** 10
    step[0, 256 + 96:256 + 128] *= 2.0 ** -10
    rows.append(step)
    rows.append(np.zeros((1, 512)))
    rows.append(-np.abs(rng.standard_normal((1, 512))))
    return np.ascontiguousarray(np.concatenate(rows, axis=0), dtype=np.float32)


UNCHANGED = ("tiny_mistral_q4_0", "tiny_mistral_q4_1", "tiny_mistral_mxfp4")


def unchanged_tokens(vocab: int):
    return [1] + [3 + (i * 37) % (vocab - 3) for i in range(7)]


def unchanged_logits(name: str) -> np.ndarray:
    """[8][vocab] logits of 8 forward steps on a fixture, on the library _lib loads"""
    from xalm_amd.model import InferenceState, Model
    from xalm_amd.xalm_file import XalmFile
    gm = Model.from_xalm(XalmFile(os.path.join(HERE, name + ".xalm")))
    st = InferenceState(gm.config)
    rows = []
    for pos, tok in enumerate(unchanged_tokens(gm.config.vocab_size)):
        gm.forward(st, tok, pos)
        rows.append(st.logits().copy())
    gm.close()
    return np.stack(rows)


def main():
    if "--unchanged" in sys.argv:
        out_dir = os.environ.get("KQ_UNCHANGED_DIR", HERE)
        os.makedirs(out_dir, exist_ok=True)
        np.savez_compressed(os.path.join(out_dir, "kq_unchanged.npz"), **{n: unchanged_logits(n) for n in UNCHANGED})
        print("kq_unchanged.npz written from", L.HIP_LIB_PATH)
        return
    sys.path.insert(0, os.environ.get("XALM_REF") or mf.REF)
    import quants  # the reference's decoders (imported from the reference checkout, not copied)

    v = golden_inputs()
    rng = np.random.default_rng(2726)
    out = {}
    for dt, name in NAMES.items():
        qt = getattr(quants.GGMLQuantizationType, name.upper())
        by = L.quantize_blocks(dt, v)
        rnd = R.random_blocks(dt, 96, rng).reshape(24, -1)
        out[name + "_values"] = v
        out[name + "_bytes"] = by
        out[name + "_random"] = rnd
        out[name + "_bytes_deq"] = np.ascontiguousarray(quants.dequantize(by, qt), dtype=np.float32)
        out[name + "_random_deq"] = np.ascontiguousarray(quants.dequantize(rnd, qt), dtype=np.float32)
    np.savez_compressed(os.path.join(HERE, "kq_golden.npz"), **out)
    print("kq_golden.npz:", {k: a.shape for k, a in out.items()})

    import hashlib
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        dst = os.path.join(td, "small_llama_q4_k_m.xalm")
        n = xalm_requant.requant(os.path.join(HERE, "small_llama_f16.xalm"), dst, "q4_k_m")
        with open(dst, "rb") as f:
            digest = hashlib.md5(f.read()).hexdigest()
        size = os.path.getsize(dst)
    with open(os.path.join(HERE, "small_llama_q4_k_m.md5"), "w") as f:
        f.write(digest + "\n")
    print(f"small_llama_q4_k_m.xalm: {n} tensors, {size} bytes, md5 {digest}")


if __name__ == "__main__":
    main()
