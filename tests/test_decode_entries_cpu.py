"""The argument checks of the six xh_decode_* and five xh_op_sample* entries without a GPU: every
context-free invalid call of tests/decode_entries_ref.py returns the code, leaves the error text and
leaves *n_done as the build before the one-driver refactor did (tests/golden/decode_entry_errors.json,
recorded by tests/golden/make_decode_entry_fixtures.py)."""
import json

import pytest

import decode_entries_ref as D
from conftest import fixture_path
from xalm_amd import _lib as L

CASES = D.cpu_cases()
with open(fixture_path("decode_entry_errors.json")) as f:
    RECORDED = json.load(f)


def test_the_table_is_the_recorded_one():
    assert sorted(RECORDED) == sorted(c[0] for c in CASES)
    # every entry has rows, and every row was rejected as invalid
    assert {(kind, e) for _, kind, e, _ in CASES} == {("decode", e) for e in D.DECODE} | {("op", e) for e in D.OPS}
    assert all(r[0] == 1 for r in RECORDED.values())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_invalid_call_reports_what_the_parent_reported(case):
    cid, kind, entry, kw = case
    assert D.run_cpu_case(L.lib(), kind, entry, kw) == RECORDED[cid], cid


def test_order_pairs_pick_the_first_check():
    """The pairs' recorded texts are those of the check that comes first, not of the second wrong argument."""
    want = {"decode seq: sampling before ctl": "bad sampling parameters", "decode adapt: ctl before trunc": "duplicate bias id",
            "decode seq: trunc before seq": "typical_p outside (0, 1]", "decode seq: seq before n_steps": "null xh_seq_ctl",
            "op ext: args before ctl": "bad sample args", "op dfa: state before stop": "state out of range",
            "op seq: seq before dfa": "no_repeat_ngram must be 0 or 2 .. XH_SEQ_MAX_MATCH"}
    for cid, text in want.items():
        assert RECORDED[cid][1] == text, cid
    # a bare XH_E_INVALID leaves the text that was there; xh_decode_greedy alone leaves *n_done too
    assert RECORDED["decode greedy: null ctx"] == [1, "null argument", -7]
    assert RECORDED["decode sample: null ctx"] == [1, "null argument", 0]
