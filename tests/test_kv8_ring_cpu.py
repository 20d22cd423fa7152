"""Ring passes on the fp8 (e4m3) KV ring without a device: the ABI surface (XH_OPT_PREFILL_RING_KV8 and
the op hook xh_op_prompt_attn_ring8).  The kernels themselves are held to the fp16 ring pass bit
for bit by tests/test_kv8_ring_gpu.py."""
import os
import re

import numpy as np

from conftest import ROOT
from test_host_cpu import declared_functions
from xalm_amd import _lib as L

HEADER = os.path.join(ROOT, "include", "xalm_hip.h")


def test_header_declares_the_option_and_the_hook():
    assert "xh_op_prompt_attn_ring8" in declared_functions(HEADER)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    enum = re.search(r"enum\s+xh_option\s*\{(.*?)\}", src, flags=re.S).group(1)
    ids = {k: int(v) for k, v in re.findall(r"(XH_OPT_\w+)\s*=\s*(\d+)", enum)}
    assert ids["XH_OPT_PREFILL_RING_KV8"] == 9
    assert len(set(ids.values())) == len(ids)  # no id is shared


def test_python_option_id():
    assert L.OPT_PREFILL_RING_KV8 == 9


def test_library_exports_the_hook():
    assert hasattr(L.lib(), "xh_op_prompt_attn_ring8")
    assert "xh_op_prompt_attn_ring8" in L._SIGNATURES
    assert callable(L.op_prompt_attn_ring8)


def test_null_pointers_are_rejected_without_a_device():
    q = np.zeros((4, 1024), np.float32)
    rc = L.lib().xh_op_prompt_attn_ring8(L.ptr(q), None, None, L.ptr(q), None, None, None, 4, 66, 66, 8, 2, 1)
    assert rc != 0
    msg = L.lib().xh_last_error(None)
    assert msg and msg.decode()
