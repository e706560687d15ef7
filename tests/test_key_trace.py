"""The sort front halves ask the device for the same things, in the same
order, as when tests/golden/key_trace.json was recorded (tests/key_trace.py
run as a script, at the commit before key resolution moved into
physical/keys.py). CPU only: a fake runtime records the calls."""
import json
from pathlib import Path

import pytest

from tests import key_trace as kt

GOLDEN = json.loads(
    (Path(__file__).parent / "golden" / "key_trace.json").read_text())
CASES = {case[0]: case for case in kt.CASES}


def test_case_list_matches_the_recording():
    assert sorted(CASES) == sorted(GOLDEN)
    assert len(CASES) >= 24


@pytest.mark.parametrize("name", sorted(CASES))
def test_trace_matches_golden(name):
    got, _ = kt.run_case(CASES[name])
    got = json.loads(json.dumps(got))  # tuples → lists, as recorded
    exp = GOLDEN[name]
    # every engine call: order, columns, specs, flags
    assert got["engine"] == exp["engine"]
    # rank columns: which are built and from what, not how often
    assert got["rank"] == exp["rank"]
    assert got["result"] == exp["result"]


@pytest.mark.parametrize("name", ["win_part_int_order_dict_refused",
                                  "win_order_dict_then_float",
                                  "sort_int_dict_refused"])
def test_rank_column_built_once_per_call(name):
    """A dictionary order key is resolved once, whichever engine ends up
    sorting: when the bucket route declines (sort_perm refused, or a float
    key beside it), the word route reuses the rank column."""
    _, runtime = kt.run_case(CASES[name])
    luts = [c for c in runtime.calls
            if c["call"] == "upload" and c.get("rank_of") == "d"]
    assert len(luts) == 1, runtime.calls
    assert luts[0]["values"] == [1, 0, 0]  # ["b", None, "a"]
    for call in ("gather", "minmax"):
        assert sum(1 for c in runtime.calls if c["call"] == call
                   and c.get("rank_of") == "d") == 1
    # and it did reach the word route
    assert any(c["call"] == "sort_word" for c in runtime.calls)
