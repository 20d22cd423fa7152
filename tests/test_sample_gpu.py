"""Seeded sampling on the device: xh_op_sample against the numpy reference (tests/sample_ref.py) and
xh_decode_sample's loop on two tiny fixtures of different weight type."""
import os
import re
import subprocess

import numpy as np
import pytest

import sample_ref as R
from conftest import ROOT, fixture_path
from xalm_amd import _lib as L
from xalm_amd.model import InferenceState, Model
from xalm_amd.xalm_file import XalmFile

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "xalm_amd", "bin", "xalm")
FIXTURES = ["tiny_mistral_f16", "tiny_mistral_f8_e4m3"]
PROMPT = [1, 84, 262, 259, 90]


@pytest.mark.parametrize("V", R.VOCABS)
def test_op_sample_matches_reference(V):
    lg = R.peaked_logits(V)
    grid = R.grid(V)
    skipped = 0
    for (t, k, p) in grid:
        an = R.grid_analysis(V, t, k, p)
        toks, kept = L.op_sample(lg, t, k, p, R.SEED, R.POS0, R.N_DRAWS)
        if not an.decided:
            skipped += 1
            continue
        assert (kept == an.n_kept).all(), (t, k, p, kept[:4], an.n_kept)
        for d in range(R.N_DRAWS):
            assert int(toks[d]) in an.accepted(R.SEED, R.POS0 + d), (t, k, p, d, int(toks[d]))
    assert skipped <= R.SKIP_CAP * len(grid)


@pytest.mark.parametrize("name", sorted(R.edge_cases()))
def test_op_sample_edge_cases(name):
    lg, t, k, p, kept_ids = R.edge_cases()[name]
    an = R.Analysis(lg, t, k, p)
    assert an.decided
    toks, kept = L.op_sample(lg, t, k, p, R.SEED, R.POS0, R.N_DRAWS)
    assert (kept == an.n_kept).all(), (kept[:4], an.n_kept)
    for d in range(R.N_DRAWS):
        assert int(toks[d]) in an.accepted(R.SEED, R.POS0 + d), (d, int(toks[d]))
    if kept_ids is not None and 0 < len(kept_ids) < 8:
        assert set(toks.tolist()) <= set(kept_ids)
        if name in ("all_equal_top3", "tie_at_kth"):  # 64 draws over 3 or 4 tokens of like weight reach each
            assert set(toks.tolist()) == set(kept_ids)


def test_op_sample_flat_logits_and_counters():
    lg = np.zeros(1000, np.float32)  # flat: only index neighbours are accepted; no top-p
    an = R.Analysis(lg, 1.0, 0, 1.0)
    toks, kept = L.op_sample(lg, 1.0, 0, 1.0, R.SEED, 0, R.N_DRAWS)
    assert (kept == 1000).all()
    for d in range(R.N_DRAWS):
        assert int(toks[d]) in an.accepted(R.SEED, d)
    # the counter is pos0 + d, taken mod 2^32; the same call twice gives the same tokens
    again, _ = L.op_sample(lg, 1.0, 0, 1.0, R.SEED, 0, R.N_DRAWS)
    assert again.tolist() == toks.tolist()
    shifted, _ = L.op_sample(lg, 1.0, 0, 1.0, R.SEED, 5, 8)
    assert shifted.tolist() == toks[5:13].tolist()
    wrapped, _ = L.op_sample(lg, 1.0, 0, 1.0, R.SEED, (3 << 32) + 5, 8)
    assert wrapped.tolist() == shifted.tolist()


# ---- the loop ----------------------------------------------------------------------------------
def hydrated(name, context=0, graphs=True):
    gm = Model.from_xalm(XalmFile(fixture_path(name + ".xalm")), context=context)
    gm.set_graphs(graphs)
    st = InferenceState(gm.config)
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    return gm, st


def replay_check(name, context, tokens, t, k, p, seed):
    """Teacher-forced replay of prompt + tokens through xh_forward: every sampled token is an
    accepted token of the reference on that step's logits at counter = its position."""
    gm, st = hydrated(name, context)
    undecided = 0
    pos = len(PROMPT)
    for tok in tokens:
        gm.get_logits(st)
        an = R.Analysis(st.logits().copy(), t, k, p)
        if an.decided:
            assert tok in an.accepted(seed, pos), (pos, tok)
        else:
            undecided += 1
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
        pos += 1
    assert undecided <= R.SKIP_CAP * len(tokens)
    gm.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_temperature_zero_is_greedy(name):
    gm, _ = hydrated(name)
    want = gm.decode_greedy(len(PROMPT), 24)
    gm.close()
    gm, _ = hydrated(name)
    assert gm.decode_sample(len(PROMPT), 24, 0.0, 7, 0.3, 99) == want
    gm.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_seeded_and_graph_independent(name):
    runs = []
    for graphs, seed in ((True, 11), (True, 11), (False, 11), (True, 12)):
        gm, _ = hydrated(name, graphs=graphs)
        runs.append(gm.decode_sample(len(PROMPT), 24, 1.5, 0, 1.0, seed))
        gm.close()
    assert len(runs[0]) == 24
    assert runs[0] == runs[1] == runs[2]
    assert runs[3] != runs[0]


@pytest.mark.parametrize("name", FIXTURES)
def test_sampled_tokens_are_accepted_by_reference(name):
    t, k, p, seed = 0.8, 40, 0.95, 5
    gm, _ = hydrated(name)
    toks = gm.decode_sample(len(PROMPT), 16, t, k, p, seed)
    gm.close()
    assert len(toks) == 16
    replay_check(name, 0, toks, t, k, p, seed)


@pytest.mark.parametrize("name", FIXTURES)
def test_one_call_equals_two(name):
    gm, _ = hydrated(name)
    whole = gm.decode_sample(len(PROMPT), 8, 1.2, 50, 1.0, 21)
    gm.close()
    gm, _ = hydrated(name)
    a = gm.decode_sample(len(PROMPT), 3, 1.2, 50, 1.0, 21)
    b = gm.decode_sample(len(PROMPT) + 3, 5, 1.2, 50, 1.0, 21)
    gm.close()
    assert a + b == whole


@pytest.mark.parametrize("name", FIXTURES)
def test_greedy_after_sample_is_unaffected(name):
    n = len(PROMPT)
    gm, st = hydrated(name)
    want = gm.decode_greedy(n, 8)
    # a sampled call, then the same state again: the greedy continuation is the same
    gm.reset()
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    sampled = gm.decode_sample(n, 5, 1.5, 0, 1.0, 3)
    gm.reset()
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    assert gm.decode_greedy(n, 8) == want
    # and greedy straight after sampled steps continues from their logits
    gm.reset()
    for pos, tok in enumerate(PROMPT):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    assert gm.decode_sample(n, 5, 1.5, 0, 1.0, 3) == sampled
    cont = gm.decode_greedy(n + 5, 6)
    gm.reset()
    for pos, tok in enumerate(PROMPT + sampled):
        gm.forward(st, tok, pos, L.OUTPUT_LOGITS)
    assert gm.decode_greedy(n + 5, 6) == cont
    gm.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_ring_wrap(name):
    t, k, p, seed = 1.0, 0, 1.0, 8
    gm, _ = hydrated(name, context=16)
    toks = gm.decode_sample(len(PROMPT), 30, t, k, p, seed)
    gm.close()
    assert len(toks) == 30
    replay_check(name, 16, toks, t, k, p, seed)


@pytest.mark.parametrize("name", FIXTURES)
def test_stop_tokens(name):
    gm, _ = hydrated(name)
    toks = gm.decode_sample(len(PROMPT), 10, 1.5, 0, 1.0, 4)
    gm.close()
    stop = toks[3]
    j = toks.index(stop)
    gm, _ = hydrated(name)
    assert gm.decode_sample(len(PROMPT), 10, 1.5, 0, 1.0, 4, stop=(stop, -1)) == toks[: j + 1]
    gm.close()


def cli_ids(*args):
    path = fixture_path("tiny_mistral_f16.xalm")
    r = subprocess.run([CLI, path, "-n", "8", "-i", "the answer is", *args], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    out = r.stdout.decode("utf-8", errors="replace")
    return [int(v) for v in re.search(r"tokens: \[([0-9,]*)\]", out).group(1).split(",")]


def test_cli_sampling():
    base = cli_ids("-g", "1")
    a = cli_ids("-t", "0.8", "-k", "40", "-s", "7", "-g", "1")
    assert len(a) == len(base) and a[: len(base) - 8] == base[: len(base) - 8]  # the prompt, then 8 ids
    assert cli_ids("-t", "0.8", "-k", "40", "-s", "7", "-g", "1") == a
    assert a != base
    assert cli_ids("-t", "0", "-k", "40", "-s", "7", "-g", "1") == base
    assert cli_ids("-t", "0", "-g", "0") == cli_ids("-g", "0")
    h = cli_ids("-t", "0.8", "-k", "40", "-s", "7", "-g", "0")  # the host Sampler::sample
    assert len(h) == len(base) and cli_ids("-t", "0.8", "-k", "40", "-s", "7", "-g", "0") == h
