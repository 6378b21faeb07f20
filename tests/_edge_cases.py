"""Inputs, cached oracle results and comparison rules for the op edge-case
tests. tests/test_ops_edges_cpu.py runs them through the CPU reference,
tests/test_ops_gpu_edges.py through the HIP kernels; both compare with
tests/_oracles.py. Helper module, not a conftest.

Every input respects the kernels' preconditions (in-range region_of/dst_off,
valid segment bounds, R >= 1 run tables, padded blobs).

Not covered: the tile grid-stride loop of field_bucket_agg_lds_kernel. It
takes a second step only past 8192 tiles of 8192 rows (67M rows), which does
not fit a test of a few seconds.
"""

import functools

import numpy as np
import torch

import _oracles as orc

AGG_TILE = 8192       # csrc/kernels.h; tests/test_hip_ops_args.py compares
LDS_CELLS = 1024
GRID_SPAN = 2048 * 256  # threads of a capped grid: n above it loops twice


# ------------------------------------------------------------ ts_bucket_agg
def _fields(rng, nf, n, nan_frac=0.1):
    f = rng.uniform(-1e6, 1e6, size=(nf, n))
    if nan_frac:
        f[rng.uniform(size=(nf, n)) < nan_frac] = np.nan
    return f


def _chunk(ts, series, fields, field_idx, lut):
    return dict(ts=np.asarray(ts, dtype=np.int64),
                series=np.asarray(series, dtype=np.int32),
                fields=np.ascontiguousarray(fields, dtype=np.float64),
                field_idx=np.asarray(field_idx, dtype=np.int32),
                lut=np.asarray(lut, dtype=np.int32))


def _sorted_rows(rng, n, n_series, t_lo, t_hi):
    series = rng.randint(-1, n_series + 2, n)
    ts = rng.randint(t_lo, t_hi, n)
    order = np.lexsort((ts, series))
    return ts[order], series[order]


def _agg_sorted(n):
    # the last rows (highest series, latest ts) pass the filters, so the
    # short last tile of n = k·AGG_TILE + 1 has a live row
    rng = np.random.RandomState(n)
    ts, series = _sorted_rows(rng, n, 18, 50_000, 900_000)
    lut = rng.randint(-1, 5, 20)
    lut[19] = 2
    return [_chunk(ts, series, _fields(rng, 3, n), [0, 1, 2], lut)], \
        (100_000, 900_000, 100_000, 50_000, 5, 16)


def _agg_unsorted_wide():
    rng = np.random.RandomState(101)
    n = 20000
    return [_chunk(rng.randint(0, 64_000, n), rng.randint(0, 40, n),
                   _fields(rng, 2, n), [0, 1], np.arange(40))], \
        (0, 64_000, 0, 1000, 40, 64)


def _agg_lds_boundary():
    # n_buckets = 1 and an identity LUT: cell == series id. Tile 0 holds ids
    # 7..1030 (1024 cells, lo = 7), tile 1 ids 1031..2055 (1025 cells), the
    # short tile 2 ids 2056..2065.
    rng = np.random.RandomState(102)
    series = np.concatenate([
        np.repeat(np.arange(7, 1031), 8),
        np.repeat(np.arange(1031, 2054), 8), np.repeat([2054, 2055], 4),
        np.repeat(np.arange(2056, 2066), 10)])
    n = len(series)
    return [_chunk(rng.randint(0, 100, n), series, _fields(rng, 2, n),
                   [0, 1], np.arange(2100))], (0, 100, 0, 100, 2100, 1)


def _agg_floor(origin, t_min, t_max):
    # ts_lo = origin - bucket_ms + 1: rows in [ts_lo, origin) pass the time
    # filter but floor to bucket -1 and must be dropped
    rng = np.random.RandomState(103 + abs(origin))
    n = 3000
    return [_chunk(rng.randint(t_min, t_max, n), rng.randint(-1, 12, n),
                   _fields(rng, 2, n), [0, 1], rng.randint(-1, 5, 10))], \
        (origin - 999, origin + 4000, origin, 1000, 5, 4)


def _agg_strided():
    rng = np.random.RandomState(104)
    n = 5000
    ts, series = _sorted_rows(rng, n, 20, 0, 1_000_000)
    fields = np.full((6, n + 37), 1e300)       # padding must never be read
    fields[:, :n] = _fields(rng, 6, n)
    return [_chunk(ts, series, fields, [3, 0, 3], rng.randint(-1, 5, 20))], \
        (100_000, 900_000, 100_000, 50_000, 5, 16)


def _agg_all_nan_cell():
    rng = np.random.RandomState(105)
    n = 600
    series = rng.randint(0, 4, n)
    fields = _fields(rng, 2, n)
    fields[1, series == 2] = np.nan
    return [_chunk(rng.randint(0, 50, n), series, fields, [0, 1],
                   np.arange(4))], (0, 100, 0, 100, 4, 1)


def _agg_no_fields():
    rng = np.random.RandomState(106)
    n = 300
    return [_chunk(rng.randint(0, 1000, n), rng.randint(0, 6, n),
                   np.zeros((1, n)), [], rng.randint(-1, 3, 6))], \
        (0, 1000, 0, 100, 3, 10)


def _agg_empty():
    return [_chunk([], [], np.zeros((2, 0)), [0, 1], [0, 1, 2])], \
        (0, 100, 0, 10, 3, 10)


def _agg_acc3():
    rng = np.random.RandomState(107)
    lut = rng.randint(-1, 5, 20)
    chunks = []
    for n, pad in ((100, 5), (8193, 0), (1, 0)):
        ts, series = _sorted_rows(rng, n, 20, 0, 1_000_000)
        fields = np.full((3, n + pad), 1e300)
        fields[:, :n] = _fields(rng, 3, n)
        chunks.append(_chunk(ts, series, fields, [2, 0], lut))
    return chunks, (100_000, 900_000, 100_000, 50_000, 5, 16)


def _agg_extremes():
    vals = [1e308, -1e308, 1e-308, -1e-308, 1.5, 5e-324, -5e-324, 0.0, -0.0]
    series = [0] * 5 + [1] * 2 + [2] * 2
    return [_chunk([10] * 9, series, np.array([vals]), [0], [0, 1, 2])], \
        (0, 100, 0, 100, 3, 1)


AGG_CASES = {
    "sorted_8191": lambda: _agg_sorted(8191),
    "sorted_8192": lambda: _agg_sorted(8192),
    "sorted_8193": lambda: _agg_sorted(8193),
    "sorted_16385": lambda: _agg_sorted(16385),
    "unsorted_wide": _agg_unsorted_wide,
    "lds_boundary": _agg_lds_boundary,
    "floor_origin_pos": lambda: _agg_floor(500, -1500, 5000),
    "floor_origin_neg": lambda: _agg_floor(-3000, -5000, 1500),
    "strided_repeat_idx": _agg_strided,
    "all_nan_cell": _agg_all_nan_cell,
    "no_fields": _agg_no_fields,
    "empty": _agg_empty,
    "acc3": _agg_acc3,
    "extremes": _agg_extremes,
}


@functools.lru_cache(maxsize=None)
def agg_case(name):
    """→ (chunks, args, oracle dict). The oracle sees the concatenation of
    the chunks (one ts_bucket_agg_acc call each)."""
    chunks, args = AGG_CASES[name]()
    idx = chunks[0]["field_idx"]
    ts = np.concatenate([c["ts"] for c in chunks])
    series = np.concatenate([c["series"] for c in chunks])
    fields = np.concatenate(
        [c["fields"][:, :len(c["ts"])] for c in chunks], axis=1)
    exp = orc.ts_bucket_agg(ts, series, fields, idx, chunks[0]["lut"], *args)
    return chunks, args, exp


def agg_cells(chunk, args):
    """Cell id per row (-1 = filtered) — only to assert that a case really
    has the tile shape it was built for."""
    ts_lo, ts_hi, origin, bucket_ms, _n_slots, n_buckets = args
    ts, se, lut = chunk["ts"], chunk["series"], chunk["lut"]
    ok = (ts >= ts_lo) & (ts < ts_hi) & (se >= 0) & (se < len(lut))
    slot = np.where(ok, lut[np.clip(se, 0, len(lut) - 1)], -1)
    b = (ts - origin) // bucket_ms
    ok &= (slot >= 0) & (b >= 0) & (b < n_buckets)
    return np.where(ok, slot * n_buckets + b, -1)


def run_agg(name, device):
    from greptimedb_amd.ops import kernels
    chunks, args, _ = agg_case(name)
    acc = None
    for c in chunks:
        t = {k: torch.as_tensor(v).to(device) for k, v in c.items()}
        acc = kernels.ts_bucket_agg_acc(
            t["ts"], t["series"], t["fields"], t["field_idx"], t["lut"],
            *args, acc=acc)
    return [o.cpu().numpy() for o in kernels.ts_bucket_agg_finish(acc)]


def check_agg(got, exp):
    """cnt/rows/min/max exact (by value: -0.0 == 0.0, NaN == NaN); sum within
    orc.sum_tol of the exact sum, per cell."""
    s, cnt, mn, mx, rows = got
    np.testing.assert_array_equal(rows, exp["rows"], err_msg="rows")
    np.testing.assert_array_equal(cnt, exp["cnt"], err_msg="cnt")
    np.testing.assert_array_equal(mn, exp["min"], err_msg="min")
    np.testing.assert_array_equal(mx, exp["max"], err_msg="max")
    assert s.shape == exp["sum"].shape
    tol = 2.0 * np.maximum(exp["cnt"] - 1, 0) * orc.U * exp["abs"]
    err = np.abs(s - exp["sum"])
    bad = ~(err <= tol) & np.isfinite(tol)
    assert not bad.any(), (
        f"sum: {int(bad.sum())} cells off, worst err/tol "
        f"{np.max(err[bad] / np.maximum(tol[bad], 5e-324))}")


# ---------------------------------------------------------- prom_range_eval
PROM_SIZES = [0, 1, 2, 127, 0, 128, 129, 130, 300, 0]
# te = -6000 + 2500·t, windows (te - 10000, te]; t = 4 is (-6000, 4000] and
# holds every sample of every segment. The offset is negative.
PROM_GRID = dict(T=8, t0=-6500, step_ms=2500, range_ms=10000, offset_ms=-500)
PROM_QS = (-0.1, 0.0, 0.37, 0.5, 1.0, 1.1)
NAN_SAFE_MODES = (orc.INSTANT, orc.LAST, orc.COUNT, orc.SUM, orc.AVG,
                  orc.MIN, orc.MAX)


def _prom_ts(rng, m):
    ts = rng.randint(-4000, 4001, m)
    # samples exactly on window ends (te: included) and begins (tb: excluded)
    ts[:4] = [-3500, 4000, 1500, -1000]
    ts[10:13] = ts[9]                      # duplicate timestamps
    return np.sort(ts)


def _gauge(rng, m):
    v = rng.uniform(-100, 100, m)
    v[20:26] = [5e-324, -5e-324, 0.0, -0.0, 2.2e-308, -2.2e-308]
    v[40] = v[41] = v[42]                  # duplicates, apart and adjacent
    v[60] = v[5]
    return v


def _counter(rng, m):
    v = np.cumsum(rng.uniform(0, 10, m))
    v[m // 3:] -= v[m // 3]                # two resets
    v[2 * m // 3:] -= v[2 * m // 3]
    return v


@functools.lru_cache(maxsize=None)
def prom_data():
    rng = np.random.RandomState(201)
    v128 = _gauge(rng, 128)
    segs = {
        1: ([4000], [7.25]),
        2: ([-3500, 1500], [-0.0, 5e-324]),
        127: (_prom_ts(rng, 127), _gauge(rng, 127)),
        128: (_prom_ts(rng, 128), v128),
        # the same 128 values plus one: both quantile selection paths
        # (cnt <= 128 and cnt > 128) see the same data
        129: (_prom_ts(rng, 129), rng.permutation(np.append(v128, 33.125))),
        # every timestamp equal: sampled == 0 and den == 0. ts - te is a
        # whole or half second in every window, so den is exactly 0
        130: (np.full(130, 1000), _counter(rng, 130)),
        300: (_prom_ts(rng, 300), _counter(rng, 300)),
    }
    ts, vals, lo, hi = [], [], [], []
    off = 0
    for m in PROM_SIZES:
        t, v = segs.get(m, ([], []))
        ts.append(np.asarray(t, dtype=np.int64))
        vals.append(np.asarray(v, dtype=np.float64))
        lo.append(off)
        hi.append(off + m)
        off += m
    ts, vals = np.concatenate(ts), np.concatenate(vals)
    lo, hi = np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64)
    # NaN variant for the modes that define NaN handling: random NaNs, a
    # leading NaN (127), an all-NaN segment (2)
    vals_nan = vals.copy()
    vals_nan[rng.uniform(size=len(vals)) < 0.15] = np.nan
    vals_nan[lo[2]:hi[2]] = np.nan
    vals_nan[lo[3]] = np.nan
    vals_nan[lo[1]] = 7.25
    return dict(ts=ts, vals=vals, vals_nan=vals_nan, lo=lo, hi=hi)


def prom_modes():
    """(id, mode, param, with_nan)"""
    out = []
    names = ["instant", "rate", "increase", "delta", "avg", "sum", "min",
             "max", "count", "last", "idelta", "irate", "deriv", "predict",
             "resets", "changes", "stddev", "stdvar", "absent", "quantile",
             "last_ts"]
    for mode, name in enumerate(names):
        if mode == orc.QUANTILE:
            out += [(f"quantile_{q}", mode, q, False) for q in PROM_QS]
        else:
            out.append((name, mode, 600.0 if mode == orc.PREDICT else 0.0,
                        False))
        if mode in NAN_SAFE_MODES:
            out.append((name + "_nan", mode, 0.0, True))
    return out


@functools.lru_cache(maxsize=None)
def prom_expected(mode, param, with_nan):
    d = prom_data()
    g = PROM_GRID
    return orc.prom_range_eval(
        d["ts"], d["vals_nan" if with_nan else "vals"], d["lo"], d["hi"],
        g["T"], g["t0"], g["step_ms"], g["range_ms"], g["offset_ms"],
        param, mode)


def run_prom(data, vals, grid, param, mode, device):
    from greptimedb_amd.ops import kernels
    t = [torch.as_tensor(a).to(device)
         for a in (data["ts"], vals, data["lo"], data["hi"])]
    return kernels.prom_range_eval(
        *t, grid["T"], grid["t0"], grid["step_ms"], grid["range_ms"],
        grid["offset_ms"], param, mode).cpu().numpy()


def check_prom(got, exp, tol, mode):
    """NaN and ±inf positions must agree. Finite values: exact for
    orc.PROM_EXACT, within the oracle's bound where it gives one (sum, avg,
    quantile), else the project's rtol = 1e-10."""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
    inf = np.isinf(exp)
    np.testing.assert_array_equal(got[inf], exp[inf])
    fin = np.isfinite(exp)
    assert np.isfinite(got[fin]).all()
    err = np.abs(got[fin] - exp[fin])
    if mode in orc.PROM_EXACT:
        bound = np.zeros_like(err)
    else:
        bound = np.where(np.isnan(tol[fin]), 1e-10 * np.abs(exp[fin]),
                         tol[fin])
    bad = ~(err <= bound)
    assert not bad.any(), (
        f"{int(bad.sum())} windows off: got {got[fin][bad][:4]}, "
        f"expected {exp[fin][bad][:4]}, bound {bound[bad][:4]}")


PROM_WIDE_GRID = dict(T=256, t0=-60000, step_ms=500, range_ms=1500,
                      offset_ms=-250)


@functools.lru_cache(maxsize=None)
def prom_wide():
    """S·T = 2100·256 > 2048·256: the kernel's grid-stride loop steps twice."""
    rng = np.random.RandomState(202)
    S = 2100
    a = rng.randint(-50000, 50000, S)
    ts = np.stack([a, a + rng.randint(0, 3000, S)], axis=1).reshape(-1)
    vals = rng.uniform(-100, 100, 2 * S)
    lo = np.arange(S, dtype=np.int64) * 2
    data = dict(ts=ts.astype(np.int64), vals=vals, lo=lo, hi=lo + 2)
    g = PROM_WIDE_GRID
    count, last = orc.prom_count_last_sorted(
        data["ts"], vals, lo, lo + 2, g["T"], g["t0"], g["step_ms"],
        g["range_ms"], g["offset_ms"])
    return data, count, last


# -------------------------------------------------------------- series_last
N_SLOTS_LAST = 15
UNBOUNDED = (-(1 << 62), 1 << 62)
BOUNDED = (-4000, 9600)


@functools.lru_cache(maxsize=None)
def series_last_case():
    """Four sources of 2000 rows: 0 and 2 sorted by (series, ts), 1 and 3
    not. → (sources [(ts, series, sorted)], lut)."""
    rng = np.random.RandomState(301)
    lut = np.arange(60) % 12            # several codes per slot
    lut[[5, 17, 40]] = -1
    lut[59] = 12                        # slot 12: mapped, but code 59 has no rows
    sources = []                        # slots 13, 14: not mapped at all
    for si, t_hi in enumerate((5000, 5000, 2500, 4000)):
        series = rng.randint(-1, 62, 2000)
        series[series == 59] = 58
        ts = rng.randint(-5000, t_hi, 2000)
        if si == 0:
            series[0], ts[0] = 3, 9000      # slot 3: tie, sorted 0 / unsorted 1
        if si == 1:
            series[777], ts[777] = 15, 9000
            series[1500], ts[1500] = 4, 9500   # slot 4: tie, unsorted 1 / sorted 2
        if si == 2:
            series[0], ts[0] = 16, 9500
            series[1], ts[1] = 6, 9700      # slot 6: two codes of one sorted
            series[2], ts[2] = 18, 9700     # source tie
        if si in (0, 2):
            order = np.lexsort((ts, series))
            series, ts = series[order], ts[order]
        sources.append((ts.astype(np.int64), series.astype(np.int32),
                        si in (0, 2)))
    return sources, lut.astype(np.int32)


@functools.lru_cache(maxsize=None)
def series_last_expected(window):
    sources, lut = series_last_case()
    return orc.series_last([(t, s) for t, s, _ in sources], lut, *window,
                           N_SLOTS_LAST)


def run_series_last(window, device):
    from greptimedb_amd.ops import kernels
    sources, lut = series_last_case()
    src = [(torch.as_tensor(t).to(device), torch.as_tensor(s).to(device), srt)
           for t, s, srt in sources]
    out = kernels.series_last(src, torch.as_tensor(lut).to(device), *window,
                              N_SLOTS_LAST)
    return [o.cpu().numpy() for o in out]


# --------------------------------------------------------------- RLE expand
def _pack_le(vals, bw):
    """values → little-endian bitstream, bw bits each."""
    v = np.asarray(vals, dtype=np.uint64)
    bits = ((v[:, None] >> np.arange(bw, dtype=np.uint64)[None, :]) & 1)
    return np.packbits(bits.astype(np.uint8).reshape(-1),
                       bitorder="little").tobytes()


def _rle_build(rng, bw, layout):
    """layout: [(is_packed, count)] → (runs i64[R,5], blob, n, values). Runs
    start on odd byte offsets with junk between them; values < 2^31."""
    top = min(1 << bw, 1 << 31)
    blob = b"\xab\xcd\xef"
    runs, values = [], []
    for is_packed, count in layout:
        start = len(values)
        if is_packed:
            v = rng.randint(0, top, count, dtype=np.int64)
            v[-1] = top - 1
            runs.append((1, len(blob), 0, start, count))
            blob += _pack_le(v, bw) + b"\xff"
            values += [int(x) for x in v]
        else:
            val = int(rng.randint(0, top))
            runs.append((0, 0, val, start, count))
            values += [val] * count
    return (np.array(runs, dtype=np.int64), blob, len(values),
            np.array(values, dtype=np.int64))


RLE_LAYOUT = [(0, 3), (1, 1), (1, 7), (0, 5), (1, 8), (1, 9), (1, 1000),
              (0, 2)]


@functools.lru_cache(maxsize=None)
def rle_case(bw):
    return _rle_build(np.random.RandomState(400 + bw), bw, RLE_LAYOUT)


@functools.lru_cache(maxsize=None)
def rle_case_big():
    return _rle_build(np.random.RandomState(433), 13, [(1, GRID_SPAN + 1)])


# ------------------------------------------------------------------ gorilla
GORILLA_N = 4096 * 2 + 5
_NAN_BITS = [0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001]


def _gorilla_ts(kind, rng, n):
    if kind == "walk":
        return 1451606400000 + np.cumsum(rng.randint(1, 20000, n))
    if kind == "const":                 # ts_bits == 0
        return np.full(n, 1700000000000)
    if kind == "minus1":                # deltas {0, -1}: ts_bits == 1
        return 1700000000000 - (np.arange(n) % 2)
    if kind == "pm1":
        return 1700000000000 + rng.randint(-1, 2, n)
    if kind == "pm2_62":                # deltas ±2^62: ts_bits 63 and 64
        ts = np.where(rng.uniform(size=n) < 0.5, 0, 1 << 62)
        ts[[0, 4096, 8192]] = [0, 1 << 62, 0]
        return ts
    if kind == "unsorted":
        return rng.randint(-10 ** 12, 10 ** 12, n)
    raise ValueError(kind)


def _gorilla_vals(kind, rng, n):
    if kind == "const":                 # val_bits == 0, scaled mode
        return np.full(n, 42.5)
    if kind == "const_raw":             # val_bits == 0, XOR mode
        return np.full(n, 0.1 + 0.2)
    if kind.startswith("scaled_"):      # exactly k decimals, negatives; the
        k = int(kind[-1])               # + 0.0 turns a rounded -0.0 into 0.0
        return np.round(rng.uniform(-500, 500, n), k) + 0.0
    if kind == "raw_special":
        v = rng.randn(n) * 1e3
        special = np.concatenate([
            np.array(_NAN_BITS, dtype=np.uint64).view(np.float64),
            [np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -0.0, 0.1 + 0.2]])
        v[::97] = np.resize(special, len(v[::97]))
        return v
    if kind == "off_grid":              # one ulp off a 4-decimal grid
        v = np.round(np.cumsum(rng.uniform(-1, 1, n)) + 50, 4)
        v[::50] = np.nextafter(v[::50], np.inf)
        v[25::50] = np.nextafter(v[25::50], -np.inf)
        return v
    raise ValueError(kind)


# (ts kind, value kind, block, pack_ts)
GORILLA_CASES = (
    [("unsorted", "raw_special", b, True) for b in (1, 2, 3, 64, 4096)] +
    [("walk", "scaled_2", b, True) for b in (1, 2, 3, 64, 4096)] +
    [("const", "const", 64, True), ("minus1", "const_raw", 64, True),
     ("minus1", "scaled_0", 3, True), ("pm1", "scaled_0", 64, True),
     ("pm2_62", "scaled_1", 64, True), ("pm2_62", "raw_special", 4096, True),
     ("walk", "scaled_3", 64, True), ("walk", "scaled_4", 4096, True),
     ("walk", "off_grid", 64, True), ("walk", "raw_special", 64, False),
     ("walk", "scaled_2", 4096, False)])


@functools.lru_cache(maxsize=None)
def gorilla_case(ts_kind, val_kind, block, pack_ts):
    """→ (ts, vals, packed) with packed = gorilla.pack(...)."""
    from greptimedb_amd.engine import gorilla
    rng = np.random.RandomState(500)
    ts = np.asarray(_gorilla_ts(ts_kind, rng, GORILLA_N), dtype=np.int64)
    vals = np.asarray(_gorilla_vals(val_kind, rng, GORILLA_N),
                      dtype=np.float64)
    return ts, vals, gorilla.pack(ts, vals, block=block, pack_ts=pack_ts)


def gorilla_headers(packed):
    """[(ts_bits, val_bits, count, val_mode, scale_k)] per block."""
    blob, block_off, _out_off, _n = packed
    return [(blob[o + 16], blob[o + 17],
             int.from_bytes(blob[o + 18:o + 20], "little"),
             blob[o + 20], blob[o + 21]) for o in map(int, block_off)]


def check_gorilla(ts, vals, packed, block, pack_ts, got_ts, got_vals):
    """Timestamps and value BIT PATTERNS must equal the inputs. A block
    packed without timestamps (pack_ts=False) decodes its base ts."""
    want_ts = ts if pack_ts else \
        np.repeat(ts[::block], block)[:len(ts)]
    np.testing.assert_array_equal(np.asarray(got_ts), want_ts)
    np.testing.assert_array_equal(
        np.ascontiguousarray(got_vals).view(np.uint64), vals.view(np.uint64))


# ------------------------------------------------- filter / dedup / scatter
SMALL_SIZES = (0, 1, 257, GRID_SPAN + 1)


@functools.lru_cache(maxsize=None)
def rows_case(n):
    """(series, ts)-sorted rows with duplicate (series, ts) groups + a LUT."""
    rng = np.random.RandomState(600 + n % 1000)
    series = rng.randint(-1, 40, n)
    ts = rng.randint(-50, 50, n)
    order = np.lexsort((ts, series))
    lut = rng.randint(-1, 5, 37)
    return (ts[order].astype(np.int64), series[order].astype(np.int32),
            lut.astype(np.int32))


def scatter_case(n, R):
    """→ inputs + per-region capacities; offsets are a shuffled, in-range,
    collision-free assignment."""
    rng = np.random.RandomState(700 + n + R)
    nf = 3
    region_of = rng.randint(0, R, n).astype(np.int32)
    dst_off = np.zeros(n, dtype=np.int64)
    caps = []
    for r in range(R):
        m = region_of == r
        caps.append(int(m.sum()) + 5)
        dst_off[m] = rng.permutation(caps[-1])[:int(m.sum())]
    return dict(ts=rng.randint(-10 ** 12, 10 ** 12, n).astype(np.int64),
                series=rng.randint(0, 1000, n).astype(np.int32),
                fields=rng.randn(nf, n), region_of=region_of,
                dst_off=dst_off), caps, nf


def run_scatter(n, R, device):
    """→ (got, expected): per-region (ts, series, fields) after the append."""
    from greptimedb_amd.ops import kernels
    c, caps, nf = scatter_case(n, R)
    e_ts = [np.full(k, -7, dtype=np.int64) for k in caps]
    e_se = [np.full(k, -7, dtype=np.int32) for k in caps]
    e_f = [np.full((nf, k), -7.0) for k in caps]
    orc.scatter_append(c["ts"], c["series"], c["fields"], c["region_of"],
                       c["dst_off"], e_ts, e_se, e_f)
    g_ts = [torch.full((k,), -7, dtype=torch.int64, device=device) for k in caps]
    g_se = [torch.full((k,), -7, dtype=torch.int32, device=device) for k in caps]
    g_f = [torch.full((nf, k), -7.0, dtype=torch.float64, device=device)
           for k in caps]
    t = {k: torch.as_tensor(v).to(device) for k, v in c.items()}
    kernels.scatter_append(t["ts"], t["series"], t["fields"], t["region_of"],
                           t["dst_off"], g_ts, g_se, g_f)
    got = [[x.cpu().numpy() for x in g] for g in (g_ts, g_se, g_f)]
    return got, [e_ts, e_se, e_f]
