"""Ring passes of the batched prompt path, the part that needs no device: the ABI surface of
XH_OPT_PREFILL_RING and xh_prefill_route.  The cutting rule itself is a function of a context's
weights and options (xh_prefill_route takes the context), so it is tested on the GPU
(tests/test_ring_prefill_gpu.py::test_route).
"""
import os
import re

from conftest import ROOT
from xalm_amd import _lib as L
from xalm_amd.model import Model


def test_route_query_and_option_are_exported():
    hdr = open(os.path.join(ROOT, "include", "xalm_hip.h")).read()
    assert re.search(r"\bXH_OPT_PREFILL_RING\s*=\s*7\b", hdr)
    assert re.search(r"\bint\s+xh_prefill_route\s*\(\s*const\s+xh_ctx\s*\*", hdr)
    assert L.OPT_PREFILL_RING == 7
    assert hasattr(L.lib(), "xh_prefill_route")
    assert "xh_prefill_route" in L._SIGNATURES and hasattr(Model, "prefill_route")


def test_route_query_rejects_a_null_context():
    # host only: an error code, no device touched, no crash
    assert L.lib().xh_prefill_route(None, 4, 0, None, None) != 0
