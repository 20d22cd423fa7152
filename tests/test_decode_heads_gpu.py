"""All six decode heads on one context, interleaved, against what the build before the one-driver refactor
produced (tests/golden/decode_heads_parent.json, recorded by tests/golden/make_decode_entry_fixtures.py
--heads): tokens, log-probability bits, final state, final mu bits and the top rows, bit for bit, with graphs
on (first pass captures every head's graph, second replays it), with graphs off, and across
xh_set_top_logprobs toggles, which drop every captured graph; and the invalid calls on a live context."""
import json

import pytest

import decode_entries_ref as D
from conftest import fixture_path

pytestmark = pytest.mark.gpu

with open(fixture_path("decode_heads_parent.json")) as f:
    RECORDED = json.load(f)


def without_top(calls):
    return [{k: v for k, v in c.items() if k != "top"} for c in calls]


def test_recorded_run_covers_every_head_twice():
    calls = RECORDED["calls"]
    assert [c["head"] for c in calls] == list(D.HEAD_ORDER + D.HEAD_ORDER[::-1])
    # every call ran its steps, or ended at the end token (the second extended call does: the stop poll's break)
    assert all(len(c["tokens"]) == D.STEPS or c["tokens"][-1] == D.EOS for c in calls), [c["tokens"] for c in calls]
    assert [len(c["tokens"]) for c in calls].count(D.STEPS) >= 11
    assert all(len(c["top"]["ids"]) == len(c["tokens"]) and len(c["top"]["ids"][0]) == 2 for c in calls)
    # the constrained calls moved the state, Mirostat moved mu
    assert calls[3]["state"] != calls[4]["state"] and calls[7]["mu"] != D.bits([6.0])[0]


@pytest.mark.parametrize("graphs", (True, False))
def test_interleaved_heads_match_the_parent(graphs):
    gm, st, dfa = D.open_model(constraint=True, graphs=graphs)
    gm.set_top_logprobs(2)
    got = D.run_heads(gm, st, dfa, top=True)
    gm.close()
    for g, w in zip(got, RECORDED["calls"]):
        assert g == w, (graphs, g["head"])
    assert len(got) == len(RECORDED["calls"])


def test_top_logprobs_toggle_recaptures_every_head():
    """Width 2 -> 0 -> 2 on one context, the whole run after each: a graph kept across a toggle would run the
    row kernel where the width is 0, or leave the top rows of another call where it is 2."""
    gm, st, dfa = D.open_model(constraint=True)
    gm.set_top_logprobs(2)
    assert D.run_heads(gm, st, dfa, top=True) == RECORDED["calls"]
    gm.set_top_logprobs(0)
    assert D.run_heads(gm, st, dfa, top=False) == without_top(RECORDED["calls"])
    gm.set_top_logprobs(2)
    assert D.run_heads(gm, st, dfa, top=True) == RECORDED["calls"]
    gm.close()


def test_invalid_calls_on_a_live_context_match_the_parent():
    gm, st, dfa = D.open_model()
    got = D.run_live_cases(gm, st, dfa)
    gm.close()
    assert sorted(got) == sorted(RECORDED["invalid"])
    for cid, want in RECORDED["invalid"].items():
        assert got[cid] == want, cid
    inv = RECORDED["invalid"]
    # what the order of the checks decides, and what only some entries check
    assert inv["sample: pos before n_steps"][1] == "negative pos" and inv["greedy: pos<0, no steps"][0] == 0
    assert inv["dfa: n_steps before constraint"][1].startswith("n_steps > ")
    assert inv["adapt: state before stop"][1].startswith("state_in ") and inv["seq: dead state, stop>=vocab"][1] == "stop token out of range"
    assert inv["adapt: unconstrained, no steps"][0] == 0 and inv["seq: unconstrained, no constraint, no steps"][0] == 0
