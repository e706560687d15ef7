"""The join asks the device for the same things, in the same order, as when
tests/golden/join_trace.json was recorded (tests/join_trace.py run as a
script, at the commit before the join's routing moved into
physical/join_plan.py). CPU only: a fake runtime records the calls."""
import json
from collections import Counter
from pathlib import Path

import pytest

from tests import join_trace as jt

GOLDEN = json.loads(
    (Path(__file__).parent / "golden" / "join_trace.json").read_text())
CASES = {case[0]: case for case in jt.CASES}


def _key(call):
    return json.dumps(call, sort_keys=True)


def test_case_list_matches_the_recording():
    assert sorted(CASES) == sorted(GOLDEN)
    assert len(CASES) >= 45


@pytest.mark.parametrize("name", sorted(CASES))
def test_trace_matches_golden(name):
    got, runtime = jt.run_case(CASES[name])
    got = json.loads(json.dumps(got))  # tuples → lists, as recorded
    exp = GOLDEN[name]
    # every engine call: order, columns, key specs, join type, flags
    assert got["engine"] == exp["engine"]
    assert got["result"] == exp["result"]
    # statistics and dictionary remaps: nothing the recording did not do (it
    # may have done more: a setup it abandoned before a side ran its WHERE)
    extra = {_key(c) for c in got["setup"]} - {_key(c) for c in exp["setup"]}
    assert not extra, extra


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_table_is_freed_once(name):
    _, runtime = jt.run_case(CASES[name])
    freed = Counter(c["table"] for c in runtime.calls
                    if c["call"] == "hash_table_free")
    assert freed == Counter(dict.fromkeys(runtime.tables, 1)), runtime.calls


def test_the_cases_reach_every_route():
    """The recording is only worth replaying if it exercises the routes."""
    seen = Counter(c["call"] for t in GOLDEN.values() for c in t["engine"])
    for call in ("materialize", "keypack", "eval", "hash_build",
                 "hash_build_cols", "filter_probe_cols",
                 "filter_probe_groupby", "hash_probe_cols", "hash_probe",
                 "hash_unmatched", "radix_join", "filter", "gather",
                 "hash_table_free"):
        assert seen[call], call
    assert any(t["setup"] for t in GOLDEN.values())
    assert sum("error" in t["result"] for t in GOLDEN.values()) >= 6
