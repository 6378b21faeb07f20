"""Shared fixtures for the grouped-quantile tests (CPU and GPU files).

* a plain per-cell ``np.quantile`` oracle for ``ops.grouped_quantile``;
* the SQL parity table: two tags, two float fields (one partly NULL), rows
  split between an SST and the memtable, (series, ts) points overwritten
  after the flush, one group whose field is entirely NULL.
"""

import numpy as np

NAN = float("nan")


def oracle(sources, field_of_sel, p_of_sel, n_cells):
    """Per-cell np.quantile loop over host copies of `sources`
    [(cell i32[n], fields f64[nf, >=n], field_idx i32[nf])].
    Returns (lo, hi, cnt, final), each [Q, n_cells]."""
    Q = len(field_of_sel)
    lo = np.full((Q, n_cells), np.nan)
    hi = np.full((Q, n_cells), np.nan)
    fin = np.full((Q, n_cells), np.nan)
    cnt = np.zeros((Q, n_cells), dtype=np.int64)
    for s in range(Q):
        cells = [np.asarray(c) for c, _f, _i in sources]
        cols = [np.asarray(f)[int(np.asarray(i)[field_of_sel[s]])][: len(c)]
                for c, f, i in sources]
        cell = np.concatenate(cells) if cells else np.zeros(0, dtype=np.int32)
        col = np.concatenate(cols) if cols else np.zeros(0)
        for c in range(n_cells):
            vals = col[cell == c]
            vals = vals[~np.isnan(vals)]
            if not len(vals):
                continue
            a = np.sort(vals)
            n = len(a)
            k1 = int(np.floor((n - 1) * p_of_sel[s]))
            cnt[s, c] = n
            lo[s, c] = a[k1]
            hi[s, c] = a[min(k1 + 1, n - 1)]
            fin[s, c] = np.quantile(a, p_of_sel[s])
    return lo, hi, cnt, fin


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ------------------------------------------------------------- SQL parity

HOUR = 3_600_000


def build_parity_table(ex, flush):
    """~200 rows in table `qt`; `flush()` persists what was inserted so far."""
    ex.execute("CREATE TABLE qt (h STRING, dc STRING, ts TIMESTAMP TIME INDEX,"
               " v DOUBLE, w DOUBLE, PRIMARY KEY (h, dc))")
    rng = np.random.default_rng(7)
    hosts = ["h0", "h1", "h2", "h3", "h4"]

    def rows(lo, hi, bump=0.0):
        out = []
        for i in range(lo, hi):
            h = hosts[i % 5]
            dc = "east" if (i // 5) % 2 == 0 else "west"
            ts = (i // 5) * 400_000 + (i % 5)          # spans ~4.4 hours
            # multiples of 1/8 and 1/2: every partial sum is exact, so avg()
            # is the same number in any summation order and can be compared
            # exactly between the two paths (and against atomics on a GPU)
            v = round(float(rng.normal(50, 20)) * 8) / 8 + bump
            # w: NULL for every row of h4 (all-NULL group) and every 3rd row
            w = "NULL" if (h == "h4" or i % 3 == 0) else \
                repr(round(float(rng.uniform(0, 10)) * 2) / 2)
            out.append(f"('{h}', '{dc}', {ts}, {v!r}, {w})")
        return ", ".join(out)

    ex.execute(f"INSERT INTO qt (h, dc, ts, v, w) VALUES {rows(0, 140)}")
    flush()
    # overwrite a few flushed (series, ts) points, then add memtable-only rows
    ex.execute(f"INSERT INTO qt (h, dc, ts, v, w) VALUES {rows(20, 32, 1000.0)}")
    ex.execute(f"INSERT INTO qt (h, dc, ts, v, w) VALUES {rows(140, 200)}")


PARITY_QUERIES = [
    "SELECT median(v) FROM qt",
    "SELECT h, approx_percentile(v, 0.8) FROM qt GROUP BY h",
    "SELECT h, date_bin('1 hour', ts) AS b, approx_percentile(v, 0.95) "
    "FROM qt GROUP BY h, b",
    "SELECT dc, approx_percentile(v, 0.5), approx_percentile(v, 0.99) AS p99, "
    "median(w), avg(v), count(*) FROM qt GROUP BY dc",
    "SELECT h, approx_percentile(w, 0.9) AS p FROM qt GROUP BY h",
    "SELECT h, dc, median(v) AS m FROM qt GROUP BY h, dc HAVING "
    "approx_percentile(v, 0.5) > 50",
    "SELECT h, approx_percentile(v, 0.9) AS p FROM qt GROUP BY h "
    "ORDER BY p DESC LIMIT 3",
    "SELECT h, median(v) FROM qt WHERE w > 5 GROUP BY h",
    "SELECT dc, median(v), count(*) FROM qt WHERE v > 900 GROUP BY dc",
    "SELECT h, median(v) FROM qt WHERE h = 'nope' GROUP BY h",
    "SELECT median(v), approx_percentile(w, 0.25) FROM qt WHERE ts < 0",
]


def _same_value(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (float, np.floating)) or isinstance(b, (float, np.floating)):
        if not (isinstance(a, (float, np.floating)) and
                isinstance(b, (float, np.floating))):
            return False
        return float(a) == float(b) or (a != a and b != b)
    return type(a) is type(b) and a == b


def assert_same_result(on, off, sql):
    assert on.names == off.names, sql
    assert list(on.kinds) == list(off.kinds), sql
    ra, rb = on.rows(), off.rows()
    assert len(ra) == len(rb), (sql, ra, rb)
    for x, y in zip(ra, rb):
        assert len(x) == len(y), sql
        for a, b in zip(x, y):
            assert _same_value(a, b), (sql, x, y)


# ------------------------------------------------------------- op cases

# (tile rows, LDS cell capacity, grid cap) of the selection kernels; the GPU
# test asserts the extension reports the same numbers.
LAUNCH_CFG = (2048, 16, 1024)
PS = [0.0, 1.0, 0.5, 0.99, 0.3, 0.7]   # n=5: p=.3 -> g=.2 (<.5), p=.7 -> g=.8


def _f(bits_):
    return np.asarray(bits_, dtype=np.uint64).view(np.float64)


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


def _groups(groups, gap=False, shuffle=None):
    """[(cell id, values)] -> (cell, vals) arrays, cells in the given order;
    `gap` puts a cell == -1 row after every row."""
    cell = np.concatenate([np.full(len(v), c, dtype=np.int32) for c, v in groups])
    vals = np.concatenate([np.asarray(v, dtype=np.float64) for _c, v in groups])
    if gap:
        c2 = np.full(2 * len(cell), -1, dtype=np.int32)
        v2 = np.full(2 * len(cell), 4.25)
        c2[::2], v2[::2] = cell, vals
        cell, vals = c2, v2
    if shuffle is not None:
        o = np.random.default_rng(shuffle).permutation(len(cell))
        cell, vals = cell[o], vals[o]
    return cell, vals


def _case(cell, vals, n_cells, ps=PS):
    return {"sources": [_src(cell, vals)], "field_of_sel": [0] * len(ps),
            "p_of_sel": list(ps), "n_cells": n_cells}


def op_cases():
    tile, cap, grid = LAUNCH_CFG
    rng = np.random.default_rng(11)
    cases = {}

    # cell sizes
    sizes = [(0, [3.5]), (1, [2.0, -1.0]), (2, [9.0, 1.0, 5.0]),
             (3, [7.5] * 10), (4, [1.0, 2.0, 2.0, 2.0, 2.0, 3.0]),
             (5, [np.nan] * 4), (6, [5.0, 1.0, 4.0, 2.0, 3.0]),
             (8, [np.nan, 6.0, np.nan, 8.0])]            # cell 7 has no rows
    cases["cell_sizes"] = _case(*_groups(sizes), 9)
    cases["cell_sizes_gaps"] = _case(*_groups(sizes, gap=True), 9)

    # keys: one deciding byte per cell
    pick = [0x00, 0x01, 0x02, 0x10, 0x7F, 0x80, 0xFE, 0xFF, 0x33]
    keys = [(0, _f([0x400921FB54442D00 | b for b in pick])),      # lowest
            (1, _f([(b << 56) | 0x0008000000000000 for b in pick]))]  # highest
    for j in range(1, 7):                                         # middle
        keys.append((1 + j, _f([0x3FF0000000000000 ^ (b << (8 * (7 - j)))
                                for b in pick])))
    keys += [(8, [-3.5, -1.0, -0.25, 0.25, 2.0, 7.0, -1e300, 1e300]),
             (9, [-np.inf, -1.0, 0.5, 3.0, np.inf]),
             (10, [5e-324, 1e-310, -5e-324, 2.2250738585072014e-308, -1e-320]),
             (11, [0.0, 0.0, 0.0]), (12, [-0.0, -0.0]),
             (13, [np.inf, np.inf]), (14, [-np.inf, 1.0])]
    cases["keys"] = _case(*_groups(keys), 15)
    cases["keys_shuffled"] = _case(*_groups(keys, shuffle=3), 15)

    # layout: sorted runs long enough for the LDS table, then the same rows
    # dealt over 300 cells in random order (global atomics)
    vals = np.round(rng.normal(0, 50, 40 * 200), 1)               # many ties
    cases["sorted_lds"] = _case(np.repeat(np.arange(40, dtype=np.int32), 200),
                                vals, 40)
    cases["shuffled_300"] = _case(rng.integers(0, 300, len(vals)).astype(np.int32),
                                  vals, 300)
    for name, ncell in (("span_cap", cap), ("span_cap_plus_1", cap + 1)):
        cell = np.sort(np.arange(tile, dtype=np.int32) % ncell)
        cases[name] = _case(cell, np.round(rng.normal(0, 5, tile), 2), ncell)
    for d in (-1, 0, 1):
        m = tile + d
        cell = (np.arange(m, dtype=np.int32) * 3) // m
        cases[f"rows_tile{d:+d}"] = _case(cell, np.round(rng.normal(0, 5, m), 2), 3)
    m = tile * grid + tile + 1              # second grid-stride step
    cases["grid_stride"] = _case((np.arange(m, dtype=np.int64) * 6 // m).astype(np.int32),
                                 np.round(rng.normal(100, 30, m), 3), 6,
                                 ps=[0.5, 0.99])
    cases["one_cell"] = _case(np.zeros(9, dtype=np.int32),
                              rng.normal(0, 1, 9), 1)

    # sources: two into one state with an empty one between; strided field
    # matrix, non-identity field_idx; Q = 3 over two fields, one used twice
    def multi(n, seed):
        r = np.random.default_rng(seed)
        cell = np.sort(r.integers(-1, 5, n)).astype(np.int32)
        cols = np.round(r.normal(0, 9, (3, n)), 1)
        cols[2, ::7] = np.nan
        return cell, cols
    c1, f1 = multi(3000, 1)
    c2, f2 = multi(1700, 2)
    cases["multi_source"] = {
        "sources": [_src(c1, f1, fidx=[2, 0], rows=(1, 4), pad=37),
                    _src(np.zeros(0, dtype=np.int32), np.zeros((3, 0)), fidx=[2, 0]),
                    _src(c2, f2, fidx=[2, 0])],
        "field_of_sel": [0, 1, 0], "p_of_sel": [0.5, 0.9, 0.99], "n_cells": 5}
    return cases


def check_op_case(ops, case, device="cpu", **kw):
    """ops.grouped_quantile + quantile_lerp against the per-cell oracle:
    lo/hi as bit patterns, cnt exactly, final values with equal_nan."""
    src = torch_sources(case, device)
    lo, hi, cnt = ops.grouped_quantile(src, case["field_of_sel"],
                                       case["p_of_sel"], case["n_cells"], **kw)
    lo, hi, cnt = lo.cpu().numpy(), hi.cpu().numpy(), cnt.cpu().numpy()
    elo, ehi, ecnt, efin = oracle(host_sources(case), case["field_of_sel"],
                                  case["p_of_sel"], case["n_cells"])
    assert np.array_equal(cnt, ecnt)
    nan = ecnt == 0
    assert np.isnan(lo[nan]).all() and np.isnan(hi[nan]).all()
    assert np.array_equal(bits(lo[~nan]), bits(elo[~nan]))
    assert np.array_equal(bits(hi[~nan]), bits(ehi[~nan]))
    fin = ops.quantile_lerp(lo, hi, cnt, case["p_of_sel"])
    assert np.array_equal(fin, efin, equal_nan=True)
