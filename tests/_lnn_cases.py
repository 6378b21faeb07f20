"""Shared cases for the last_non_null merge tests (CPU and GPU files).

* ``cases()``: named ``(series i32[n], ts i64[n], fields f64[nf, n])`` inputs,
  already (series, ts, seq)-sorted, each with the answer of ``oracle`` — a
  plain per-group Python loop that shares nothing with ``ops.cpu_ref``;
* ``check``: compares an op result with that answer bit for bit (so NaN
  positions and ``-0.0`` count);
* the SQL script of the merge-mode scenario and its expected rows.
"""

import functools

import numpy as np

NAN = float("nan")


def oracle(series, ts, fields):
    """(kidx i64[g], merged f64[nf, g]) by walking every group backwards."""
    n = len(ts)
    nf = fields.shape[0]
    kidx = [i for i in range(n)
            if i == n - 1 or series[i] != series[i + 1] or ts[i] != ts[i + 1]]
    merged = np.empty((nf, len(kidx)), dtype=np.float64)
    start = 0
    for j, last in enumerate(kidx):
        for f in range(nf):
            merged[f, j] = fields[f, last]
            for r in range(last, start - 1, -1):
                if not np.isnan(fields[f, r]):
                    merged[f, j] = fields[f, r]
                    break
        start = last + 1
    return np.asarray(kidx, dtype=np.int64), merged


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _from_lengths(lengths, nf, rng, p_nan=0.4, ts_of=None):
    """Rows for groups of the given lengths: one series per 7 groups, ts
    ascending inside a series, values random with NaNs at rate p_nan."""
    lengths = np.asarray(lengths, dtype=np.int64)
    gid = np.repeat(np.arange(len(lengths)), lengths)
    series = (gid // 7).astype(np.int32)
    ts = ((gid % 7) * 1000).astype(np.int64) if ts_of is None else ts_of(gid)
    n = len(gid)
    fields = rng.normal(0, 100, size=(nf, n))
    fields[rng.random((nf, n)) < p_nan] = NAN
    return series, ts, fields


def _build():
    out = {}
    z = np.zeros
    out["n0"] = (z(0, np.int32), z(0, np.int64), z((3, 0)))
    out["n1"] = (z(1, np.int32), z(1, np.int64), np.array([[1.5], [NAN]]))
    out["nf0"] = (np.array([0, 0, 1], np.int32), np.array([5, 5, 5], np.int64),
                  z((0, 3)))

    rng = np.random.default_rng(20261021)
    # every group one row: the output is the input, NaNs included
    se, ts, f = _from_lengths(np.ones(1000, np.int64), 3, rng)
    out["all_len1"] = (se, ts, f)
    # ~5000 rows, random group lengths 1..5, random NaN patterns
    se, ts, f = _from_lengths(rng.integers(1, 6, size=1700), 3, rng)
    out["random_1_5"] = (se, ts, f)
    # long groups straddling wave (64) and block (256) boundaries: the odd
    # single-row groups in front shift every long group's first and last row
    # off a multiple of 64; mostly NaN so the look-back really walks them
    lens = [1, 1, 1, 63, 1, 64, 65, 1, 1, 255, 256, 1, 257, 3, 64, 63, 2]
    se, ts, f = _from_lengths(lens, 2, rng, p_nan=0.97)
    out["wave_block_edges"] = (se, ts, f)

    # one 70,000-row group between small ones
    before = [1, 3, 2]
    after = [2, 1, 4]
    lens = before + [70_000] + after
    se, ts, f = _from_lengths(lens, 3, rng, p_nan=0.3)
    lo = sum(before)
    hi = lo + 70_000
    f[:, lo:hi] = NAN
    f[0, lo] = 11.0            # field 0: only the group's first row
    f[1, hi - 1] = 22.0        # field 1: only its last row
    f[2, lo - 2:lo] = 33.0     # field 2: all NaN here, the group before is not
    out["long_group"] = (se, ts, f)

    # same ts / different series next to same series / different ts
    out["adjacent_keys"] = (
        np.array([0, 0, 0, 1, 1, 2, 2, 2], np.int32),
        np.array([5, 5, 6, 5, 6, 6, 6, 7], np.int64),
        np.array([[1.0, NAN, NAN, 2.0, NAN, 3.0, NAN, NAN],
                  [NAN, NAN, 4.0, NAN, 5.0, NAN, 6.0, NAN]]))
    # +-inf and -0.0 are values, not nulls; a -0.0 must keep its sign bit
    inf = float("inf")
    out["inf_negzero"] = (
        np.array([0, 0, 0, 1, 1, 1, 2, 2], np.int32),
        np.array([1, 1, 1, 1, 1, 1, 1, 1], np.int64),
        np.array([[inf, NAN, NAN, -0.0, NAN, NAN, 0.0, -0.0],
                  [1.0, -inf, NAN, 0.0, -0.0, NAN, NAN, NAN]]))
    return out


@functools.lru_cache(maxsize=1)
def cases():
    """{name: (series, ts, fields, kidx, merged)}; built once per process and
    shared, so callers must not write into the arrays."""
    out = {}
    for name, (se, ts, f) in _build().items():
        kidx, merged = oracle(se, ts, f)
        for a in (se, ts, f, kidx, merged):
            a.setflags(write=False)
        out[name] = (se, ts, f, kidx, merged)
    return out


CASE_NAMES = ["n0", "n1", "nf0", "all_len1", "random_1_5", "wave_block_edges",
              "long_group", "adjacent_keys", "inf_negzero"]


def check(got_kidx, got_merged, kidx, merged):
    got_kidx = np.asarray(got_kidx)
    got_merged = np.asarray(got_merged)
    assert got_kidx.dtype == np.int64 and got_merged.dtype == np.float64
    np.testing.assert_array_equal(got_kidx, kidx)
    assert got_merged.shape == merged.shape
    np.testing.assert_array_equal(bits(got_merged), bits(merged))


# ------------------------------------------------------------- SQL scenario

CREATE_LNN = ("CREATE TABLE lnn (host STRING, ts TIMESTAMP TIME INDEX, "
              "cpu DOUBLE, memory DOUBLE, PRIMARY KEY (host)) "
              "WITH ('merge_mode'='last_non_null')")
CREATE_LR = ("CREATE TABLE lr (host STRING, ts TIMESTAMP TIME INDEX, "
             "cpu DOUBLE, memory DOUBLE, PRIMARY KEY (host)) "
             "WITH ('merge_mode'='last_row')")

# (statement suffix after "INSERT INTO <t> VALUES ", expected lnn rows after it,
#  expected last_row rows after it); rows are (host, ts, cpu, memory)
STEPS = [
    ("('host1', 0, 0, NULL), ('host2', 1, NULL, 1)",
     [("host1", 0, 0.0, None), ("host2", 1, None, 1.0)],
     [("host1", 0, 0.0, None), ("host2", 1, None, 1.0)]),
    ("('host1', 0, NULL, 10), ('host2', 1, 11, NULL)",
     [("host1", 0, 0.0, 10.0), ("host2", 1, 11.0, 1.0)],
     [("host1", 0, None, 10.0), ("host2", 1, 11.0, None)]),
    ("('host1', 0, 20, NULL)",
     [("host1", 0, 20.0, 10.0), ("host2", 1, 11.0, 1.0)],
     [("host1", 0, 20.0, None), ("host2", 1, 11.0, None)]),
    ("('host1', 0, NULL, NULL)",
     [("host1", 0, 20.0, 10.0), ("host2", 1, 11.0, 1.0)],
     [("host1", 0, None, None), ("host2", 1, 11.0, None)]),
]


def _cell(v):
    if v is None:
        return None
    if isinstance(v, (float, np.floating)):
        return None if np.isnan(v) else float(v)
    if hasattr(v, "timestamp"):               # datetime-like
        return int(round(v.timestamp() * 1000))
    if isinstance(v, (int, np.integer)):
        return int(v)
    return v


def select_rows(ex, table, where=""):
    r = ex.execute(f"SELECT host, ts, cpu, memory FROM {table} {where} "
                   "ORDER BY host, ts")
    return [tuple(_cell(c[i]) for c in r.columns)
            for i in range(len(r.columns[0]) if r.columns else 0)]
