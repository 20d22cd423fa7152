#!/usr/bin/env python
"""Re-quantize the weight matrices of an .xalm file to a block type of this build.

    tools/xalm_requant.py IN.xalm OUT.xalm --type mxfp4

Every 2-D ``*.weight`` tensor of an f32 / f16 / bf16 file whose rows are whole blocks (32 elements;
the K-quants q4_k / q6_k: 256) goes through xh_quantize_blocks (the host quantizer,
include/xalm_synth.h); norm weights, tokenizer tensors and anything else are copied through byte for
byte, and so is a 2-D weight whose columns are no whole number of blocks (the tool names each).
``--type q4_k_m`` is the recipe of that name: Q6_K for ``embed``, ``output`` and every ``mlp.down``,
Q4_K for the rest (so q / k / v and gate / up keep one dtype each).  The header is rewritten in the
container layout xalm_amd/xalm_file.py documents: u64 header size (4096-aligned), the JSON, zero
padding, then the tensor data at 32-byte aligned offsets.  A re-quantized tensor's header shape is
[rows, bytes per row] and its ``hash`` the md5 of its new bytes (no reader checks it).
"""
import argparse
import hashlib
import json
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from xalm_amd import _lib as L  # noqa: E402
from xalm_amd.xalm_file import XalmFile  # noqa: E402

TYPES = {"mxfp4": L.MXFP4, "q8_0": L.Q8_0, "q4_0": L.Q4_0, "q4_1": L.Q4_1, "q5_0": L.Q5_0, "q5_1": L.Q5_1,
         "q4_k": L.Q4_K, "q6_k": L.Q6_K}
RECIPES = ("q4_k_m",)


def tensor_type(type_name: str, name: str) -> str:
    """The block type `type_name` gives the tensor `name` (a recipe picks per tensor)."""
    if type_name == "q4_k_m":
        return "q6_k" if name.startswith(("embed.", "output.")) or ".mlp.down." in name else "q4_k"
    return type_name
FLOAT_TYPES = ("F32", "F16", "BF16")


def to_f32(raw: np.ndarray, type_name: str) -> np.ndarray:
    if type_name == "F32":
        return raw.view(np.float32)
    if type_name == "F16":
        return raw.view(np.float16).astype(np.float32)
    return (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)  # BF16


def requant(src: str, dst: str, type_name: str) -> int:
    xf = XalmFile(src)
    with open(src, "rb") as f:
        (hsize,) = struct.unpack("<Q", f.read(8))
        header = json.loads(f.read(hsize - 8).split(b"\0", 1)[0].decode("utf-8"))
    tensors = header[xf.arch]["tensors"]
    blobs, off, n_done = [], 0, 0
    for name, t in tensors.items():
        ti = xf.tensors[name]
        raw = np.ascontiguousarray(xf.raw(name))
        tname = tensor_type(type_name, name)
        elems, nbytes = L.block_geometry(TYPES[tname])
        is_weight = ti.type in FLOAT_TYPES and len(ti.shape) == 2 and name.endswith(".weight")
        if is_weight and ti.shape[1] % elems:
            print(f"{name}: {ti.shape[1]} columns are no whole {elems}-element blocks of {tname}, copied unchanged")
        elif is_weight:
            w = to_f32(raw, ti.type).reshape(ti.shape)
            raw = L.quantize_blocks(TYPES[tname], w).reshape(-1)
            t["type"] = tname
            t["shape"] = [ti.shape[0], ti.shape[1] // elems * nbytes]
            t["hash"] = hashlib.md5(raw.tobytes()).hexdigest()
            n_done += 1
        t["offset"] = off
        t["size"] = int(raw.size)
        blobs.append((off, raw))
        off = (off + raw.size + 31) & ~31
    js = json.dumps(header).encode("utf-8")
    new_hsize = (8 + len(js) + 1 + 4095) & ~4095
    with open(dst, "wb") as f:
        f.write(struct.pack("<Q", new_hsize))
        f.write(js)
        f.write(b"\0" * (new_hsize - 8 - len(js)))
        for o, raw in blobs:
            f.seek(new_hsize + o)
            f.write(raw.tobytes())
    return n_done


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--type", default="mxfp4", choices=sorted(TYPES) + list(RECIPES))
    a = ap.parse_args()
    n = requant(a.src, a.dst, a.type)
    print(f"{a.dst}: {n} tensors re-quantized to {a.type}, {os.path.getsize(a.dst)} bytes")


if __name__ == "__main__":
    main()
