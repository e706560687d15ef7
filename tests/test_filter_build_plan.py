"""Build-from-columns routing (physical/filter_build.py) as a pure function
of plan facts: TPC-H Q3's two joins, every declining shape, the knob, the cap
and the row minimum. No device."""
import pytest

from dask_sql_amd.physical import filter_build as fb

RADIX = 8_000_000


def _v(**kw):
    facts = dict(join_type="inner", fusable=True, pend_l=False, pend_r=False,
                 n_l=1000, n_r=1000, probe_side=None, radix_min_build=RADIX,
                 cap=fb.DEFAULT_MAX_ROWS, knob_off=False, keys_int=True,
                 key_rewritten=False, n_cols=1, max_cols=16)
    facts.update(kw)
    return fb.verdict(**facts)


def test_q3_customer_orders_join():
    """customer (1.5 M, WHERE pending) x orders (15 M, WHERE pending): orders
    probes, customer builds and stays pending; two columns (segment, key)."""
    v = _v(pend_l=True, pend_r=True, n_l=1_500_000, n_r=15_000_000,
           probe_side="r", n_cols=2)
    assert v and v.side == "l" and v.pending


def test_q3_orders_lineitem_join():
    """the first join's 1.46 M rows (materialized) x lineitem (60 M, WHERE
    pending): an empty predicate over the join output's key column."""
    v = _v(pend_l=False, pend_r=True, n_l=1_460_000, n_r=59_986_052,
           probe_side="r", n_cols=1)
    assert v and v.side == "l" and not v.pending


@pytest.mark.parametrize("join_type,n_l,n_r,side", [
    ("inner", 10, 20, "l"), ("inner", 20, 10, "r"), ("inner", 10, 10, "r"),
    ("left", 10, 20, "r"), ("leftanti", 10, 20, "r"), ("right", 20, 10, "l"),
])
def test_build_side_without_a_probe_verdict(join_type, n_l, n_r, side):
    assert fb.build_side(join_type, None, n_l, n_r) == side
    v = _v(join_type=join_type, n_l=n_l, n_r=n_r)
    assert v and v.side == side and not v.pending  # materialized: any type


def test_build_side_opposite_the_filter_probe_side():
    assert fb.build_side("inner", "l", 10, 20) == "r"
    assert fb.build_side("inner", "r", 20, 10) == "l"


def test_pending_build_side_without_pending_probe():
    v = _v(pend_r=True, n_l=30_000, n_r=1000)
    assert v and v.side == "r" and v.pending


@pytest.mark.parametrize("join_type", ["left", "right", "leftanti"])
def test_declines_non_inner_with_pending_build(join_type):
    n_l, n_r = (1000, 30_000) if join_type == "right" else (30_000, 1000)
    side = fb.build_side(join_type, None, n_l, n_r)
    v = _v(join_type=join_type, n_l=n_l, n_r=n_r,
           pend_l=side == "l", pend_r=side == "r")
    assert not v and "pending build side" in v.reason
    # the same join with the WHERE already run builds from columns
    assert _v(join_type=join_type, n_l=n_l, n_r=n_r)


def test_declines_too_many_columns():
    assert _v(pend_r=True, n_l=30_000, n_cols=16)
    v = _v(pend_r=True, n_l=30_000, n_cols=17)
    assert not v and "columns" in v.reason
    assert not _v(n_cols=17)  # a materialized side cannot exceed it, but …


def test_declines_non_integer_key():
    v = _v(keys_int=False)
    assert not v and "integer" in v.reason
    assert not _v(keys_int=False, pend_r=True, n_l=30_000)


def test_declines_rewritten_build_key():
    v = _v(key_rewritten=True)
    assert not v and "dictionary" in v.reason
    assert not _v(key_rewritten=True, pend_r=True, n_l=30_000)


def test_declines_radix_gate():
    v = _v(pend_l=True, pend_r=True, n_l=RADIX, n_r=4 * RADIX,
           probe_side=None, cap=10 * RADIX)
    assert not v and "radix" in v.reason
    # radix off: the gate is gone
    assert _v(pend_l=True, pend_r=True, n_l=RADIX, n_r=4 * RADIX,
              probe_side="r", cap=10 * RADIX, radix_min_build=None)
    # a materialized build side is the radix path's own business
    assert _v(n_l=RADIX, n_r=4 * RADIX)


def test_declines_unfusable_join():
    v = _v(fusable=False, pend_r=True, n_l=30_000)
    assert not v and "fused" in v.reason


def test_cap():
    cap = fb.DEFAULT_MAX_ROWS
    assert _v(pend_l=True, n_l=cap, n_r=10 * cap, probe_side="r")
    v = _v(pend_l=True, n_l=cap + 1, n_r=10 * cap, probe_side="r")
    assert not v and "DSX_FILTERBUILD_MAX_ROWS" in v.reason
    # the cap binds a pending side only
    assert _v(n_l=cap + 1, n_r=10 * cap, probe_side="r")


def test_row_minimum():
    """Builds below it keep keypack + hash_build, pending or not; the count
    is the build side's (base rows of a pending side), not the probe's."""
    m = fb.DEFAULT_MIN_ROWS
    assert 1500 < m <= 1 << 20  # Q3 at benchmark size is above it
    v = _v(min_rows=m, n_l=m - 1, n_r=100 * m, probe_side="r")
    assert not v and "DSX_FILTERBUILD_MIN_ROWS" in v.reason and v.side == "l"
    assert not _v(min_rows=m, n_l=m - 1, n_r=100 * m, probe_side="r",
                  pend_l=True, pend_r=True)
    assert _v(min_rows=m, n_l=m, n_r=100 * m, probe_side="r")
    v = _v(min_rows=m, n_l=m, n_r=100 * m, probe_side="r", pend_l=True)
    assert v and v.pending
    assert _v(min_rows=m, n_l=100 * m, n_r=m, probe_side="l")
    # Q3's two joins at benchmark size
    assert _v(min_rows=m, pend_l=True, pend_r=True, n_l=1_500_000,
              n_r=15_000_000, probe_side="r", n_cols=2)
    assert _v(min_rows=m, pend_r=True, n_l=1_460_000, n_r=59_986_052,
              probe_side="r")


def test_row_minimum_env(monkeypatch):
    monkeypatch.delenv("DSX_FILTERBUILD_MIN_ROWS", raising=False)
    assert fb.min_rows() == fb.DEFAULT_MIN_ROWS
    monkeypatch.setenv("DSX_FILTERBUILD_MIN_ROWS", "0")
    assert fb.min_rows() == 0
    monkeypatch.setenv("DSX_FILTERBUILD_MIN_ROWS", "x")
    assert fb.min_rows() == fb.DEFAULT_MIN_ROWS


def test_cap_env(monkeypatch):
    monkeypatch.delenv("DSX_FILTERBUILD_MAX_ROWS", raising=False)
    assert fb.max_rows() == fb.DEFAULT_MAX_ROWS
    monkeypatch.setenv("DSX_FILTERBUILD_MAX_ROWS", "123")
    assert fb.max_rows() == 123
    monkeypatch.setenv("DSX_FILTERBUILD_MAX_ROWS", "x")
    assert fb.max_rows() == fb.DEFAULT_MAX_ROWS


def test_knob(monkeypatch):
    monkeypatch.delenv("DSX_DISABLE_FILTERBUILD", raising=False)
    assert not fb.disabled()
    monkeypatch.setenv("DSX_DISABLE_FILTERBUILD", "0")
    assert not fb.disabled()
    monkeypatch.setenv("DSX_DISABLE_FILTERBUILD", "1")
    assert fb.disabled()
    v = _v(knob_off=True)
    assert not v and v.reason == "DSX_DISABLE_FILTERBUILD"
    assert not _v(knob_off=True, pend_r=True, n_l=30_000)
