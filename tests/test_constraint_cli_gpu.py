"""`xalm -R <regex>` through the CLI on the tiny f16 fixture: the host route (-g 0: Sampler::sample
over xh_constraint_mask) and the device route (-g 1: xh_decode_sample_dfa) print the same ids for a
seed, and the generated text matches the expression."""
import os
import re
import subprocess

import pytest

from conftest import ROOT, fixture_path
from xalm_amd import _lib as L
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "xalm_amd", "bin", "xalm")
FIXTURE = fixture_path("tiny_mistral_f16.xalm")
EOS = 2
# at most 6 * 2 + 5 + 1 tokens and the end token: every run ends within -n 32
PATTERN = r"(of|to)( (of|to)){5}[.?]"


def cli(*args):
    r = subprocess.run([CLI, FIXTURE, "-n", "32", "-i", "the answer is", *args], capture_output=True, timeout=120)
    out = r.stdout.decode("utf-8", errors="replace")
    ids = re.search(r"tokens: \[([0-9,]*)\]", out)
    return r.returncode, out, [int(v) for v in ids.group(1).split(",")] if ids else None, r.stderr.decode(errors="replace")


@pytest.mark.parametrize("sampling", [("-t", "0"), ("-t", "0.9", "-k", "40", "-p", "0.95", "-s", "11"),
                                      ("-t", "0", "-r", "1.3", "-w", "8"), ("-t", "1.2", "-M", "0.05", "-s", "3")])
def test_host_and_device_routes_agree(sampling):
    n_prompt = len(cli("-n", "1", "-g", "1")[2]) - 1
    pieces = L.token_pieces(XalmFile(FIXTURE).tokens())
    runs = {}
    for g in ("0", "1"):
        rc, out, ids, err = cli("-R", PATTERN, "-g", g, *sampling)
        assert rc == 0, err
        gen = ids[n_prompt:]
        assert gen[-1] == EOS and EOS not in gen[:-1], gen
        text = b"".join(pieces[t] for t in gen[:-1])
        assert re.fullmatch(PATTERN.encode(), text), text
        assert text.decode() in out, (out[:200], text)   # what was printed is that text
        runs[g] = ids
    assert runs["0"] == runs["1"]
    # the constraint did something: the unconstrained run's text does not match
    _, _, free, _ = cli("-g", "1", *sampling)
    assert not re.fullmatch(PATTERN.encode(), b"".join(pieces[t] for t in free[n_prompt:] if t != EOS))


def test_bad_expression_is_an_error():
    rc, _, ids, err = cli("-R", "(of", "-g", "1")
    assert rc != 0 and ids is None and "-R" in err
