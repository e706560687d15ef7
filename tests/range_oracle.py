"""sqlite3 as the oracle for RANGE window frames, shared by
test_window_range_lowering.py (host model) and test_gpu_window_range.py
(device). Not a test module.

A bound is ``("unb",)``, ``("cur",)`` or ``("off", x)`` with a signed
offset: negative PRECEDING, positive FOLLOWING, zero PRECEDING on the low
side and FOLLOWING on the high side."""
import sqlite3

import numpy as np
import pandas as pd

UNB = ("unb",)
CUR = ("cur",)


def OFF(x):
    return ("off", x)


def bound_sql(b, side, fmt=None):
    if b[0] == "unb":
        return "UNBOUNDED " + ("PRECEDING" if side == "lo" else "FOLLOWING")
    if b[0] == "cur":
        return "CURRENT ROW"
    x = b[1]
    txt = fmt(abs(x)) if fmt else str(abs(x))
    if x < 0 or (x == 0 and side == "lo"):
        return f"{txt} PRECEDING"
    return f"{txt} FOLLOWING"


def frame_sql(lo, hi, fmt=None):
    return (f"RANGE BETWEEN {bound_sql(lo, 'lo', fmt)} AND "
            f"{bound_sql(hi, 'hi', fmt)}")


def bound_rank(b, side):
    """Order of bound kinds in a frame: a low bound of a later kind than
    the high bound is refused."""
    if b[0] == "unb":
        return 0 if side == "lo" else 4
    if b[0] == "cur":
        return 2
    x = b[1]
    return 1 if (x < 0 or (x == 0 and side == "lo")) else 3


def legal(lo, hi):
    return bound_rank(lo, "lo") <= bound_rank(hi, "hi")


EXPR = {"sum": "SUM(v)", "count": "COUNT(v)", "countstar": "COUNT(*)",
        "avg": "AVG(v)", "min": "MIN(v)", "max": "MAX(v)",
        "first": "FIRST_VALUE(w)", "last": "LAST_VALUE(w)"}


def over_sql(lo, hi, desc=False, nulls_first=False, partition=True,
             order="o", fmt=None, spell_nulls=True):
    """The OVER clause. sqlite's default NULL placement differs from the
    engine's (NULLs last in both directions), so it is spelled out."""
    txt = ("PARTITION BY p " if partition else "") + f"ORDER BY {order}"
    if desc:
        txt += " DESC"
    if spell_nulls or nulls_first:
        txt += " NULLS FIRST" if nulls_first else " NULLS LAST"
    return txt + " " + frame_sql(lo, hi, fmt)


def query(table, funcs, over):
    cols = ", ".join(f"{EXPR[f]} OVER ({over}) AS {f}" for f in funcs)
    return f"SELECT rid, {cols} FROM {table}"


class SqliteTable:
    """One table in an in-memory sqlite database. NA / NaN become NULL."""

    def __init__(self, name, df):
        self.name = name
        self.n = len(df)
        self.db = sqlite3.connect(":memory:")
        cols = list(df.columns)
        self.db.execute(f"CREATE TABLE {name} ({', '.join(cols)})")
        rows = []
        arrays = []
        for c in cols:
            s = df[c]
            a = s.astype(object).where(s.notna(), None).tolist()
            arrays.append([x.item() if isinstance(x, np.generic) else x
                           for x in a])
        rows = list(zip(*arrays))
        self.db.executemany(
            f"INSERT INTO {name} VALUES ({', '.join('?' * len(cols))})", rows)

    def run(self, funcs, over):
        """→ {func: float64 array in rid order, NaN = NULL}"""
        cur = self.db.execute(query(self.name, funcs, over))
        rows = cur.fetchall()
        assert len(rows) == self.n
        out = {f: np.full(self.n, np.nan) for f in funcs}
        for row in rows:
            for f, x in zip(funcs, row[1:]):
                if x is not None:
                    out[f][row[0]] = float(x)
        return out


def f64(series):
    return pd.Series(series).to_numpy(dtype=np.float64, na_value=np.nan)


def assert_same(got, want, what):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(np.isnan(got) != np.isnan(want))
    assert bad.size == 0, f"{what}: NULL positions differ at rows {bad[:8]}"
    ok = ~np.isnan(want)
    bad = np.flatnonzero(ok)[got[ok] != want[ok]]
    assert bad.size == 0, (f"{what}: values differ at rows {bad[:8]}: "
                           f"{got[bad[:8]]} vs {want[bad[:8]]}")
