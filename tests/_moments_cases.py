"""Shared cases and checkers for the grouped-moments tests (CPU and GPU files).

* op cases for ``ops.grouped_moments`` with a plain per-cell numpy oracle;
* the tolerances, derived from each case's own data (see ``bounds``);
* the SQL parity table and its queries, each with a description of what it
  computes so that the expected values come from numpy over the inserted rows.
"""

import numpy as np

U = 2.0 ** -53
AGG_TILE = 8192          # rows per tile of the moments kernels
LDS_CELLS = 1024         # cell span a tile may accumulate in LDS
KINDS = ["var_pop", "var_samp", "stddev_pop", "stddev_samp",
         "covar_pop", "covar_samp", "covar", "corr"]
PLANES = ["n", "mean_x", "mean_y", "m2x", "m2y", "cxy", "const_x", "const_y"]


# ------------------------------------------------------------- tolerances

def bounds(n, A, m2x, m2y):
    """Allowed |difference| between two correct evaluations of the planes of
    one cell with n pairs, A = max(|x|, |y|) and the given sums of squares.

    Means: a sum of n terms in any order is off by at most n*u*sum|x|, so the
    mean by n*u*A, twice for two evaluations, with slack: 4*n*u*A.
    m2: first-order bound for n non-negative terms in any order, with slack
    for the subtraction and the product, 8*n*u*m2; plus the effect of the
    mean's own error d, which enters only as n*d^2 because sum(x - mean) = 0.
    cxy: the same with sum|dx*dy| <= sqrt(m2x*m2y) (Cauchy-Schwarz).
    corr: cxy's bound divided by sqrt(m2x*m2y)."""
    n = np.asarray(n, dtype=np.float64)
    e2 = n * (4 * n * U * A) ** 2
    g = np.sqrt(m2x * m2y)
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = 8 * n * U + np.where(g > 0, e2 / g, 0.0)
    return {"mean": 4 * n * U * A, "m2x": 8 * n * U * m2x + e2,
            "m2y": 8 * n * U * m2y + e2, "cxy": 8 * n * U * g + e2,
            "corr": corr}


def value_bound(kind, n, A, m2x, m2y, value):
    """`bounds` carried through the final division and square root of SQL
    aggregate `kind`; `value` is the (reference) result. Each division and
    sqrt adds one rounding (u * |value|) per evaluation. For the square root
    |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(a) and also <= sqrt(|a - b|)."""
    b = bounds(n, A, m2x, m2y)
    if kind == "corr":
        return float(b["corr"])
    den = n if kind.endswith("_pop") else n - 1
    if kind.startswith("covar"):
        return float(b["cxy"] / den + 2 * U * abs(value))
    dvar = float(b["m2x"] / den)
    if kind.startswith("var"):
        return dvar + 2 * U * abs(value)
    sd = abs(value)                       # stddev: value = sqrt(var)
    dsd = min(dvar / sd, np.sqrt(dvar)) if sd > 0 else np.sqrt(dvar)
    return float(dsd + 4 * U * sd)


# ------------------------------------------------------------- op cases

def _src(cell, cols, fidx=None, rows=None, pad=0):
    """One source: `cols` [nf_total, n]; `rows`=(r0, r1) + `pad` make the
    field matrix a strided view base[r0:r1, :n] of a wider, taller base."""
    cols = np.atleast_2d(np.asarray(cols, dtype=np.float64))
    n = cols.shape[1]
    if rows is None:
        base, rows = cols, (0, cols.shape[0])
    else:
        base = np.full((rows[1] + 1, n + pad), 123.0)
        base[rows[0]:rows[1], :n] = cols
    fidx = np.arange(cols.shape[0]) if fidx is None else fidx
    return {"cell": np.asarray(cell, dtype=np.int32), "base": base,
            "rows": rows, "n": n, "fidx": np.asarray(fidx, dtype=np.int32)}


def host_sources(case):
    return [(s["cell"], s["base"][s["rows"][0]:s["rows"][1], :s["n"]], s["fidx"])
            for s in case["sources"]]


def torch_sources(case, device):
    import torch
    out = []
    for s in case["sources"]:
        base = torch.from_numpy(np.ascontiguousarray(s["base"])).to(device)
        out.append((torch.from_numpy(s["cell"]).to(device),
                    base[s["rows"][0]:s["rows"][1], :s["n"]],
                    torch.from_numpy(s["fidx"]).to(device)))
    return out


def _case(sources, sels, n_cells):
    if isinstance(sources, dict):
        sources = [sources]
    return {"sources": sources, "fx": [s[0] for s in sels],
            "fy": [s[1] for s in sels], "n_cells": n_cells}


ALL4 = [(0, 0), (0, 1), (1, 1), (1, 0)]


def op_cases():
    rng = np.random.default_rng(23)
    T = AGG_TILE
    cases = {}

    n = 3 * T + 17
    cases["sorted_lds"] = _case(
        _src((np.arange(n, dtype=np.int64) * 40 // n).astype(np.int32),
             rng.normal(5, 3, (2, n))), ALL4, 40)

    n = 20_000                                     # 3000 cells > LDS_CELLS
    cases["unsorted_global"] = _case(
        _src(rng.integers(0, 3000, n).astype(np.int32),
             rng.normal(0, 10, (2, n))), [(0, 1), (1, 1)], 3000)

    # cell 0 ends exactly at row T; cell 1 spans tiles 1, 2 and 3
    n = 3 * T + 500
    cell = np.zeros(n, dtype=np.int32)
    cell[T:3 * T + 100] = 1
    cell[3 * T + 100:] = 2
    cases["straddle"] = _case(_src(cell, rng.normal(-2, 7, (2, n))), ALL4, 3)

    nan = np.nan
    x = [1.0, nan, 2.0, nan, 4.0, 7.5,   nan, 3.0, nan,   nan, 5.0, 1.0,
         2.0, nan, 9.0]
    y = [2.0, 1.0, nan, nan, 3.0, -1.0,  1.0, nan, nan,   2.0, 6.0, nan,
         8.0, 3.0, -4.0]
    cell = [0] * 6 + [1] * 3 + [2] * 3 + [3] * 3    # cell 4: no rows
    cases["nan_pairs"] = _case(_src(cell, [x, y]), ALL4, 5)

    n = 2 * T + 100
    cell = (np.arange(n, dtype=np.int64) * 10 // n).astype(np.int32)
    cell[::3] = -1
    cell[[T - 1, T, 2 * T - 1, 2 * T, n - 1]] = -1
    cases["filtered"] = _case(_src(cell, rng.normal(1, 2, (2, n))), ALL4, 10)

    n = 4 * 300
    cell = np.repeat(np.arange(4, dtype=np.int32), 300)
    cols = rng.normal(3, 1, (2, n))
    cols[0, (cell == 0) | (cell == 2)] = 0.1        # sum / n != 0.1 in general
    cases["constant"] = _case(_src(cell, cols), [(0, 0), (0, 1), (1, 0)], 4)

    n = 8 * 1000
    cell = np.repeat(np.arange(8, dtype=np.int32), 1000)
    x = 1e9 + rng.normal(0, 1, n)
    y = -3e8 + 0.5 * (x - 1e9) + rng.normal(0, 1, n)
    cases["offset"] = _case(_src(cell, [x, y]), [(0, 1), (0, 0), (1, 1)], 8)

    def multi(n, seed):
        r = np.random.default_rng(seed)
        cell = np.sort(r.integers(-1, 5, n)).astype(np.int32)
        cols = r.normal(0, 9, (3, n))
        cols[2, ::7] = np.nan
        return cell, cols
    c1, f1 = multi(3000, 1)
    c2, f2 = multi(9000, 2)
    # field_idx orders differ: selection field 0 is column 2 in both, stored
    # in another row of each source's matrix
    cases["multi_source"] = _case(
        [_src(c1, f1[[1, 2, 0]], fidx=[1, 2], rows=(1, 4), pad=37),
         _src(np.zeros(0, dtype=np.int32), np.zeros((3, 0)), fidx=[2, 0]),
         _src(c2, f2, fidx=[2, 0])],
        [(0, 1), (0, 0), (1, 0)], 5)
    return cases


LDS_VARIANTS = ["sorted_lds", "straddle", "multi_source"]


def _pairs(case, s):
    """Valid (cell, x, y) rows of selection s over all sources."""
    cs, xs, ys = [], [], []
    for cell, f, fidx in host_sources(case):
        cs.append(cell)
        xs.append(f[fidx[case["fx"][s]]][:len(cell)])
        ys.append(f[fidx[case["fy"][s]]][:len(cell)])
    c, x, y = np.concatenate(cs), np.concatenate(xs), np.concatenate(ys)
    ok = (c >= 0) & (c < case["n_cells"]) & ~np.isnan(x) & ~np.isnan(y)
    return c[ok], x[ok], y[ok]


def oracle(case):
    """Planes by the textbook definition, one numpy call per cell, plus the
    per-cell A = max(|x|, |y|) the tolerances need."""
    M, C = len(case["fx"]), case["n_cells"]
    out = {"n": np.zeros((M, C), dtype=np.int64),
           "mean_x": np.full((M, C), np.nan), "mean_y": np.full((M, C), np.nan),
           "m2x": np.zeros((M, C)), "m2y": np.zeros((M, C)),
           "cxy": np.zeros((M, C)),
           "const_x": np.zeros((M, C), dtype=bool),
           "const_y": np.zeros((M, C), dtype=bool), "A": np.zeros((M, C))}
    for s in range(M):
        c, x, y = _pairs(case, s)
        order = np.argsort(c, kind="stable")
        c, x, y = c[order], x[order], y[order]
        ids, starts = np.unique(c, return_index=True)
        for ci, a, b in zip(ids, starts, np.append(starts[1:], len(c))):
            xs, ys = x[a:b], y[a:b]
            k = b - a
            out["n"][s, ci] = k
            out["mean_x"][s, ci] = np.mean(xs)
            out["mean_y"][s, ci] = np.mean(ys)
            out["const_x"][s, ci] = np.min(xs) == np.max(xs)
            out["const_y"][s, ci] = np.min(ys) == np.max(ys)
            out["m2x"][s, ci] = 0.0 if out["const_x"][s, ci] else np.var(xs) * k
            out["m2y"][s, ci] = 0.0 if out["const_y"][s, ci] else np.var(ys) * k
            both = out["const_x"][s, ci] or out["const_y"][s, ci]
            out["cxy"][s, ci] = 0.0 if both else \
                np.sum((xs - np.mean(xs)) * (ys - np.mean(ys)))
            out["A"][s, ci] = max(np.abs(xs).max(), np.abs(ys).max())
    return out


_ORACLES: dict = {}


def oracle_of(name, case):
    if name not in _ORACLES:
        _ORACLES[name] = oracle(case)
    return _ORACLES[name]


def check_planes(got, ref, A):
    """`got` and `ref`: the 8 planes as numpy arrays, PLANES order."""
    from greptimedb_amd.ops import cpu_ref
    g = dict(zip(PLANES, [np.asarray(p) for p in got]))
    r = dict(zip(PLANES, [np.asarray(ref[k]) for k in PLANES]))
    assert g["n"].dtype == np.int64 and g["const_x"].dtype == bool
    for k in ("n", "const_x", "const_y"):
        assert np.array_equal(g[k], r[k]), k
    b = bounds(r["n"], A, r["m2x"], r["m2y"])
    has = r["n"] > 0
    for k in ("mean_x", "mean_y"):
        assert np.isnan(g[k][~has]).all(), k
        d = np.abs(g[k][has] - r[k][has])
        assert (d <= b["mean"][has]).all(), (k, d.max())
    for k in ("m2x", "m2y", "cxy"):
        d = np.abs(g[k] - r[k])
        assert (d <= b[k]).all(), (k, float((d - b[k]).max()))
    # a constant column: sums of squares exactly zero
    assert (g["m2x"][g["const_x"]] == 0.0).all()
    assert (g["m2y"][g["const_y"]] == 0.0).all()
    assert (g["cxy"][g["const_x"] | g["const_y"]] == 0.0).all()
    for kind in KINDS:
        gv, gn = cpu_ref.moments_finish(kind, [g[k] for k in PLANES])
        rv, rn = cpu_ref.moments_finish(kind, [r[k] for k in PLANES])
        assert np.array_equal(gn, rn), kind
        assert np.isnan(gv[gn]).all(), kind
        if kind == "corr":
            assert gn[g["const_x"] | g["const_y"]].all()
            d = np.abs(gv[~gn] - rv[~rn])
            assert (d <= b["corr"][~gn]).all(), (kind, d.max())
            assert (np.abs(gv[~gn]) <= 1.0).all()


def run_op_case(ops, case, device="cpu", **kw):
    planes = ops.grouped_moments(torch_sources(case, device), case["fx"],
                                 case["fy"], case["n_cells"], **kw)
    assert len(planes) == 8
    M, C = len(case["fx"]), case["n_cells"]
    assert all(tuple(p.shape) == (M, C) for p in planes)
    if device != "cpu":
        assert all(p.is_cuda for p in planes)
    return [p.cpu().numpy() for p in planes]


# ------------------------------------------------------------- SQL parity

HOUR = 3_600_000
HOSTS = ["h0", "h1", "h2", "h3", "h4"]


def build_moments_table(ex, flush, name="mt", lnn=False):
    """~200 rows in table `name`: tags h, dc; float fields a, b (b constant
    for h3) and c (NULL for all of h4 and every third row). Part of it is
    flushed, a few flushed points are overwritten afterwards. Returns the
    visible rows as dicts, after the table's merge rule on (h, dc, ts)."""
    ex.execute(f"CREATE TABLE {name} (h STRING, dc STRING, ts TIMESTAMP TIME "
               f"INDEX, a DOUBLE, b DOUBLE, c DOUBLE, PRIMARY KEY (h, dc))"
               + (" WITH ('merge_mode'='last_non_null')" if lnn else ""))
    rng = np.random.default_rng(17)
    visible = {}

    def rows(lo, hi, bump=0.0):
        out = []
        for i in range(lo, hi):
            h = HOSTS[i % 5]
            dc = "east" if (i // 5) % 2 == 0 else "west"
            ts = (i // 5) * 400_000 + (i % 5)            # spans ~4.4 hours
            # multiples of 1/8: sums are exact, so avg() is the same number
            # in any summation order and compares exactly between the paths
            a = round(float(rng.normal(50, 20)) * 8) / 8 + bump
            b = 2.5 if h == "h3" else \
                a / 2 + round(float(rng.normal(0, 5)) * 8) / 8
            c = None if (h == "h4" or i % 3 == 0) else \
                round(float(rng.uniform(0, 10)) * 8) / 8
            old = visible.get((h, dc, ts), {})
            if c is None and lnn:          # last_non_null keeps the older c
                c_seen = old.get("c")
            else:
                c_seen = c
            visible[(h, dc, ts)] = {"h": h, "dc": dc, "ts": ts, "a": a,
                                    "b": b, "c": c_seen}
            out.append(f"('{h}', '{dc}', {ts}, {a!r}, {b!r}, "
                       f"{'NULL' if c is None else repr(c)})")
        return ", ".join(out)

    ins = f"INSERT INTO {name} (h, dc, ts, a, b, c) VALUES "
    ex.execute(ins + rows(0, 140))
    flush()
    ex.execute(ins + rows(20, 32, 100.0))
    ex.execute(ins + rows(140, 200))
    return list(visible.values())


def _h(r):
    return (r["h"],)


def _b(r):
    return (r["ts"] // HOUR * HOUR,)


def _hb(r):
    return (r["h"], r["ts"] // HOUR * HOUR)


def _dc(r):
    return (r["dc"],)


# sql; key: row -> group key, equal to the first len(key) output columns;
# where: row filter; cols: output column -> (kind, x, y), or ("cv", x) for
# stddev_samp(x) / avg(x); having / top: see check_sql_numpy. Columns not in
# `cols` are ordinary aggregates and must agree exactly between the paths.
SQL_CASES = [
    dict(sql="SELECT var_pop(a), var_samp(a), stddev_pop(a), stddev_samp(a), "
             "covar_pop(a, b), covar_samp(a, b), covar(a, b), corr(a, b) FROM mt",
         key=lambda r: (),
         cols={0: ("var_pop", "a", "a"), 1: ("var_samp", "a", "a"),
               2: ("stddev_pop", "a", "a"), 3: ("stddev_samp", "a", "a"),
               4: ("covar_pop", "a", "b"), 5: ("covar_samp", "a", "b"),
               6: ("covar", "a", "b"), 7: ("corr", "a", "b")},
         plan="Plan: grouped-moments (two-pass, M=2, cells=1)"),
    dict(sql="SELECT h, corr(a, b), corr(a, c), var_samp(c), covar_pop(c, a) "
             "FROM mt GROUP BY h",
         key=_h, cols={1: ("corr", "a", "b"), 2: ("corr", "a", "c"),
                       3: ("var_samp", "c", "c"), 4: ("covar_pop", "c", "a")},
         plan="Plan: grouped-moments (two-pass, M=4, cells=5)"),
    dict(sql="SELECT date_bin('1 hour', ts) AS t, stddev_samp(a), covar(a, c) "
             "FROM mt GROUP BY t",
         key=_b, cols={1: ("stddev_samp", "a", "a"), 2: ("covar", "a", "c")}),
    dict(sql="SELECT h, date_bin('1 hour', ts) AS t, stddev_pop(b), corr(b, a), "
             "var_pop(c) FROM mt GROUP BY h, t",
         key=_hb, cols={2: ("stddev_pop", "b", "b"), 3: ("corr", "b", "a"),
                        4: ("var_pop", "c", "c")}),
    # residual filter on a field; every rewritten point passes it in its new
    # version (a is redrawn around 150), so no older version can show through
    dict(sql="SELECT h, stddev_samp(a), corr(a, b) FROM mt WHERE a > 40 GROUP BY h",
         key=_h, where=lambda r: r["a"] > 40,
         cols={1: ("stddev_samp", "a", "a"), 2: ("corr", "a", "b")}),
    dict(sql="SELECT h, dc, var_samp(a) AS v FROM mt GROUP BY h, dc "
             "HAVING var_samp(a) > 500",
         key=lambda r: (r["h"], r["dc"]), cols={2: ("var_samp", "a", "a")},
         having=(2, lambda v: v > 500)),
    dict(sql="SELECT h, stddev_samp(a) AS s FROM mt GROUP BY h "
             "ORDER BY s DESC LIMIT 3",
         key=_h, cols={1: ("stddev_samp", "a", "a")}, top=(1, 3)),
    dict(sql="SELECT dc, corr(a, b) AS r, avg(a), max(b), count(*), count(c), "
             "approx_percentile(a, 0.9), stddev_samp(c) FROM mt GROUP BY dc",
         key=_dc, cols={1: ("corr", "a", "b"), 7: ("stddev_samp", "c", "c")},
         plan="Plan: grouped-quantile (radix select, Q=1, cells=2, moments M=2)"),
    dict(sql="SELECT h, stddev_samp(a) / avg(a) AS cv FROM mt GROUP BY h",
         key=_h, cols={1: ("cv", "a")}),
    dict(sql="SELECT h, var_pop(c), corr(c, a) FROM mt WHERE h = 'h4' GROUP BY h",
         key=_h, where=lambda r: r["h"] == "h4",
         cols={1: ("var_pop", "c", "c"), 2: ("corr", "c", "a")}),
]


def group_stats(rows, case):
    """{group key: {column: (expected value or None, bound)}} by numpy over
    the inserted rows."""
    groups: dict = {}
    for r in rows:
        if case.get("where") is None or case["where"](r):
            groups.setdefault(case["key"](r), []).append(r)
    out = {}
    for key, rs in groups.items():
        out[key] = {}
        for col, spec in case["cols"].items():
            kind = "stddev_samp" if spec[0] == "cv" else spec[0]
            fx = spec[1]
            fy = spec[2] if len(spec) > 2 else spec[1]
            pairs = [(r[fx], r[fy]) for r in rs
                     if r[fx] is not None and r[fy] is not None]
            x = np.array([p[0] for p in pairs], dtype=np.float64)
            y = np.array([p[1] for p in pairs], dtype=np.float64)
            out[key][col] = _numpy_value(kind, x, y)
            if spec[0] == "cv" and out[key][col][0] is not None:
                v, tol = out[key][col]
                avg = float(np.mean(x))
                out[key][col] = (v / avg, tol / abs(avg) + 2 * U * abs(v / avg))
    return out


def _numpy_value(kind, x, y):
    n = len(x)
    need = 1 if kind.endswith("_pop") else 2
    if n < need:
        return None, 0.0
    ddof = 0 if kind.endswith("_pop") else 1
    if kind == "corr":
        if x.min() == x.max() or y.min() == y.max():
            return None, 0.0
        v = float(np.corrcoef(x, y)[0, 1])
    elif kind.startswith("covar"):
        v = float(np.cov(x, y, ddof=ddof)[0, 1]) if n > ddof else None
    elif kind.startswith("var"):
        v = float(np.var(x, ddof=ddof))
    else:
        v = float(np.std(x, ddof=ddof))
    A = max(np.abs(x).max(), np.abs(y).max())
    m2x = float(np.var(x) * n)
    m2y = float(np.var(y) * n)
    return v, value_bound(kind, n, A, m2x, m2y, v)


def _key_of(row, nkey):
    return tuple(int(v) if isinstance(v, (int, np.integer)) else v
                 for v in row[:nkey])


def check_sql_numpy(res, rows, case):
    """`res` against numpy over the inserted rows: groups, NULLs, values."""
    want = group_stats(rows, case)
    nkey = len(next(iter(want))) if want else 0
    if "having" in case:
        col, pred = case["having"]
        want = {k: v for k, v in want.items()
                if v[col][0] is not None and pred(v[col][0])}
    got = res.rows()
    keys = [_key_of(r, nkey) for r in got]
    if "top" in case:
        col, k = case["top"]
        ranked = sorted((kv for kv in want.items() if kv[1][col][0] is not None),
                        key=lambda kv: -kv[1][col][0])
        assert keys == [kv[0] for kv in ranked[:k]], case["sql"]
    else:
        assert keys == sorted(want), (case["sql"], keys)
    for key, r in zip(keys, got):
        for col, (v, tol) in want[key].items():
            if v is None:
                assert r[col] is None, (case["sql"], key, col, r[col])
            else:
                assert r[col] is not None and abs(float(r[col]) - v) <= tol, \
                    (case["sql"], key, col, r[col], v, tol)


def check_sql_same(on, off, rows, case):
    """Device plan against host path: names, kinds, row order and NULLs the
    same; moment columns within the derived bound, every other column equal."""
    sql = case["sql"]
    want = group_stats(rows, case)
    nkey = len(next(iter(want))) if want else 0
    assert on.names == off.names, sql
    assert list(on.kinds) == list(off.kinds), sql
    ra, rb = on.rows(), off.rows()
    assert len(ra) == len(rb), (sql, ra, rb)
    for x, y in zip(ra, rb):
        key = _key_of(x, nkey)
        assert key == _key_of(y, nkey), (sql, x, y)
        for col, (a, b) in enumerate(zip(x, y)):
            assert (a is None) == (b is None), (sql, x, y)
            if a is None:
                continue
            if col in case["cols"]:
                tol = want[key][col][1]
                assert abs(float(a) - float(b)) <= tol, (sql, col, a, b, tol)
            else:
                assert a == b, (sql, col, a, b)
