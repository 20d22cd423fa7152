"""Record what the decode entries did before their host path became one driver (tests/decode_entries_ref.py
holds the tables and the run; this script only writes what they return).

* ``decode_entry_errors.json``: return code, error text and ``*n_done`` of every context-free invalid call of
  the six ``xh_decode_*`` and five ``xh_op_sample*`` entries.  No GPU needed.
* ``decode_heads_parent.json`` (``--heads``, needs a GPU): the twelve interleaved calls of all six heads on
  ``tiny_mistral_f16.xalm`` with graphs on and ``xh_set_top_logprobs`` 2 (tokens, log-probability bits, final
  state, final mu bits, top rows), and the invalid calls on a live context.

Both were recorded ONCE from a build of the commit before the refactor
(``XALM_HIP_LIB=<that build's libxalm_hip.so> python tests/golden/make_decode_entry_fixtures.py [--heads]``):
what tests/test_decode_entries_cpu.py and tests/test_decode_heads_gpu.py hold the entries to.  Do not
regenerate them from a later build.  ``DECODE_FIXTURE_DIR`` names another output directory.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import decode_entries_ref as D  # noqa: E402
from xalm_amd import _lib as L  # noqa: E402


def write(name, obj):
    out_dir = os.environ.get("DECODE_FIXTURE_DIR", HERE)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, name), "w") as f:
        json.dump(obj, f, indent=0, sort_keys=True)
        f.write("\n")
    print(name, "written from", L.HIP_LIB_PATH)


def heads():
    gm, st, dfa = D.open_model()
    invalid = D.run_live_cases(gm, st, dfa)
    gm.close()
    gm, st, dfa = D.open_model(constraint=True)
    gm.set_top_logprobs(2)
    calls = D.run_heads(gm, st, dfa, top=True)
    gm.close()
    write("decode_heads_parent.json", dict(calls=calls, invalid=invalid))


def main():
    if "--heads" in sys.argv:
        return heads()
    lib = L.lib()
    write("decode_entry_errors.json", {cid: D.run_cpu_case(lib, kind, entry, kw) for cid, kind, entry, kw in D.cpu_cases()})


if __name__ == "__main__":
    main()
