#!/usr/bin/env python
"""Re-quantize the weight matrices of an .xalm file to a block type of this build.

    tools/xalm_requant.py IN.xalm OUT.xalm --type mxfp4

Every 2-D ``*.weight`` tensor of an f32 / f16 / bf16 file whose rows are whole 32-element blocks
goes through xh_quantize_blocks (the host quantizer, include/xalm_synth.h); norm weights, tokenizer
tensors and anything else are copied through byte for byte.  The header is rewritten in the
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

TYPES = {"mxfp4": L.MXFP4, "q8_0": L.Q8_0, "q4_0": L.Q4_0, "q4_1": L.Q4_1, "q5_0": L.Q5_0, "q5_1": L.Q5_1}
FLOAT_TYPES = ("F32", "F16", "BF16")


def to_f32(raw: np.ndarray, type_name: str) -> np.ndarray:
    if type_name == "F32":
        return raw.view(np.float32)
    if type_name == "F16":
        return raw.view(np.float16).astype(np.float32)
    return (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)  # BF16


def requant(src: str, dst: str, type_name: str) -> int:
    dtype = TYPES[type_name]
    xf = XalmFile(src)
    with open(src, "rb") as f:
        (hsize,) = struct.unpack("<Q", f.read(8))
        header = json.loads(f.read(hsize - 8).split(b"\0", 1)[0].decode("utf-8"))
    tensors = header[xf.arch]["tensors"]
    blobs, off, n_done = [], 0, 0
    for name, t in tensors.items():
        ti = xf.tensors[name]
        raw = np.ascontiguousarray(xf.raw(name))
        if (ti.type in FLOAT_TYPES and len(ti.shape) == 2 and name.endswith(".weight") and ti.shape[1] % 32 == 0):
            w = to_f32(raw, ti.type).reshape(ti.shape)
            raw = L.quantize_blocks(dtype, w).reshape(-1)
            t["type"] = type_name
            t["shape"] = [ti.shape[0], ti.shape[1] // 32 * L.GQ_BLOCK_BYTES[dtype]]
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
    ap.add_argument("--type", default="mxfp4", choices=sorted(TYPES))
    a = ap.parse_args()
    n = requant(a.src, a.dst, a.type)
    print(f"{a.dst}: {n} tensors re-quantized to {a.type}, {os.path.getsize(a.dst)} bytes")


if __name__ == "__main__":
    main()
