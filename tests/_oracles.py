"""Independent oracles for the op edge-case tests.

Plain Python / numpy, one row or one window at a time, exact sums through
math.fsum. Nothing here imports greptimedb_amd.ops: both the HIP kernels and
their torch reference (ops.cpu_ref) are checked against this module, so a
mistake shared by those two still shows. Helper module, not a conftest.
"""

import math

import numpy as np

NAN = float("nan")
U = 2.0 ** -53          # unit roundoff of f64


def sum_tol(k, abs_sum):
    """Recursive-summation bound for k addends in any order,
    |err| <= (k-1)·u·Σ|v|, doubled for a two-level (tile, then global)
    accumulation."""
    return 2.0 * max(k - 1, 0) * U * abs_sum


def _abs_sum(vals):
    try:
        return math.fsum(abs(v) for v in vals)
    except OverflowError:
        return math.inf


# ------------------------------------------------------------ ts_bucket_agg
def ts_bucket_agg(ts, series, fields, field_idx, slot_lut, ts_lo, ts_hi,
                  origin, bucket_ms, n_slots, n_buckets):
    """Per-row loop, floor bucket (Python //). Returns a dict of arrays:
    sum/cnt/min/max/abs [nf, n_slots, n_buckets], rows [n_slots, n_buckets];
    abs is Σ|v| per cell (for sum_tol)."""
    nf = len(field_idx)
    cells = [[[] for _ in range(n_slots * n_buckets)] for _ in range(nf)]
    rows = np.zeros((n_slots, n_buckets), dtype=np.int64)
    for i in range(len(ts)):
        t = int(ts[i])
        if not (ts_lo <= t < ts_hi):
            continue
        s = int(series[i])
        if not (0 <= s < len(slot_lut)):
            continue
        slot = int(slot_lut[s])
        if slot < 0:
            continue
        b = (t - origin) // bucket_ms
        if not (0 <= b < n_buckets):
            continue
        rows[slot, b] += 1
        for f in range(nf):
            v = float(fields[int(field_idx[f])][i])
            if v != v:
                continue
            cells[f][slot * n_buckets + b].append(v)
    shape = (nf, n_slots, n_buckets)
    out = {"sum": np.zeros(shape), "cnt": np.zeros(shape, dtype=np.int64),
           "min": np.full(shape, NAN), "max": np.full(shape, NAN),
           "abs": np.zeros(shape), "rows": rows}
    for f in range(nf):
        for c, vals in enumerate(cells[f]):
            if not vals:
                continue
            ix = (f, c // n_buckets, c % n_buckets)
            out["cnt"][ix] = len(vals)
            out["min"][ix] = min(vals)
            out["max"][ix] = max(vals)
            out["abs"][ix] = _abs_sum(vals)
            try:
                out["sum"][ix] = math.fsum(vals)
            except OverflowError:
                out["sum"][ix] = NAN     # abs is inf there: sum unchecked
    return out


# ---------------------------------------------------------- prom_range_eval
(INSTANT, RATE, INCREASE, DELTA, AVG, SUM, MIN, MAX, COUNT, LAST, IDELTA,
 IRATE, DERIV, PREDICT, RESETS, CHANGES, STDDEV, STDVAR, ABSENT, QUANTILE,
 LAST_TS) = range(21)

PROM_EXACT = {INSTANT, LAST, LAST_TS, COUNT, ABSENT, MIN, MAX, RESETS,
              CHANGES, IDELTA}


def _skipnan(fn, w):
    ok = [v for v in w if v == v]
    return fn(ok) if ok else NAN


def _window(mode, wt, w, tb, te, range_ms, param):
    """One window: (value, abs tolerance or None). None = exact for the
    PROM_EXACT modes, the project's rtol for the rest."""
    cnt = len(w)
    if mode in (INSTANT, LAST):
        return (w[-1] if cnt else NAN), None
    if mode == LAST_TS:
        return (float(wt[-1]) if cnt else NAN), None
    if mode == COUNT:
        return (float(cnt) if cnt else NAN), None
    if mode == ABSENT:
        return (NAN if cnt else 1.0), None
    if cnt == 0:
        return NAN, None
    if mode in (SUM, AVG):
        s = math.fsum(w)
        tol = sum_tol(cnt, _abs_sum(w))
        return (s, tol) if mode == SUM else (s / cnt, tol / cnt)
    if mode == MIN:
        return _skipnan(min, w), None
    if mode == MAX:
        return _skipnan(max, w), None
    if mode in (STDDEV, STDVAR):
        mean = math.fsum(w) / cnt
        var = math.fsum((v - mean) ** 2 for v in w) / cnt
        return (var if mode == STDVAR else math.sqrt(var)), None
    if mode in (RESETS, CHANGES):
        k = 0
        for p, v in zip(w, w[1:]):
            k += (v < p) if mode == RESETS else (v != p)
        return float(k), None
    if mode == QUANTILE:
        if param < 0:
            return -math.inf, None
        if param > 1:
            return math.inf, None
        sw = sorted(w)
        rank = param * (cnt - 1)
        k1 = int(math.floor(rank))
        k2 = min(k1 + 1, cnt - 1)
        r = sw[k1] + (sw[k2] - sw[k1]) * (rank - k1)
        # one rounding of difference from FMA contraction of the interpolation
        return r, 2.0 * 2.0 ** -52 * max(abs(sw[k1]), abs(sw[k2]))
    if cnt < 2:
        return NAN, None
    if mode in (RATE, INCREASE, DELTA):
        counter = mode != DELTA
        total = w[-1] - w[0]
        if counter:
            total = math.fsum([total] + [p for p, v in zip(w, w[1:]) if v < p])
        sampled = (wt[-1] - wt[0]) / 1000.0
        avg_dur = sampled / (cnt - 1)
        to_start = (wt[0] - tb) / 1000.0
        to_end = (te - wt[-1]) / 1000.0
        if counter and total > 0 and w[0] >= 0:
            to_start = min(to_start, sampled * (w[0] / total))
        thresh = avg_dur * 1.1
        ext = sampled
        ext += to_start if to_start < thresh else avg_dur / 2
        ext += to_end if to_end < thresh else avg_dur / 2
        r = total * (ext / sampled if sampled > 0 else 1.0)
        if mode == RATE:
            r /= range_ms / 1000.0
        return r, None
    if mode in (IDELTA, IRATE):
        dv = w[-1] - w[-2]
        if mode == IDELTA:
            return dv, None
        dt = (wt[-1] - wt[-2]) / 1000.0
        d = w[-1] if w[-1] < w[-2] else dv
        return (d / dt if dt > 0 else NAN), None
    if mode in (DERIV, PREDICT):
        x = [(t - te) / 1000.0 for t in wt]
        n = float(cnt)
        sx, sy = math.fsum(x), math.fsum(w)
        sxx = math.fsum(a * a for a in x)
        sxy = math.fsum(a * b for a, b in zip(x, w))
        den = n * sxx - sx * sx
        if den == 0:
            return NAN, None
        slope = (n * sxy - sx * sy) / den
        if mode == DERIV:
            return slope, None
        return (sy - slope * sx) / n + slope * param, None
    raise ValueError(mode)


def prom_range_eval(ts, vals, seg_lo, seg_hi, T, t0, step_ms, range_ms,
                    offset_ms, param, mode):
    """Per-window loop over (tb, te]. Returns (out[S,T], tol[S,T]); tol is NaN
    where the mode's own rule applies (exact, or the project rtol)."""
    S = len(seg_lo)
    out = np.full((S, T), NAN)
    tol = np.full((S, T), NAN)
    for s in range(S):
        seg_t = [int(x) for x in ts[int(seg_lo[s]):int(seg_hi[s])]]
        seg_v = [float(x) for x in vals[int(seg_lo[s]):int(seg_hi[s])]]
        for t in range(T):
            te = t0 + t * step_ms - offset_ms
            tb = te - range_ms
            idx = [j for j, x in enumerate(seg_t) if tb < x <= te]
            r, e = _window(mode, [seg_t[j] for j in idx],
                           [seg_v[j] for j in idx], tb, te, range_ms, param)
            out[s, t] = r
            if e is not None:
                tol[s, t] = e
    return out, tol


def prom_count_last_sorted(ts, vals, seg_lo, seg_hi, T, t0, step_ms,
                           range_ms, offset_ms):
    """count_over_time / last_over_time for many segments at once: sample x
    is in window t iff x <= te[t] < x + range, an interval of the sorted te
    grid found with np.searchsorted. Segments must be ts-sorted."""
    S = len(seg_lo)
    te = t0 + np.arange(T, dtype=np.int64) * step_ms - offset_ms
    seg_of = np.repeat(np.arange(S), np.asarray(seg_hi) - np.asarray(seg_lo))
    first = np.searchsorted(te, ts, "left")
    end = np.searchsorted(te, ts + range_ms, "left")
    diff = np.zeros((S, T + 1), dtype=np.int64)
    np.add.at(diff, (seg_of, first), 1)
    np.add.at(diff, (seg_of, end), -1)
    cnt = np.cumsum(diff, axis=1)[:, :T]
    last = np.full((S, T), NAN)
    for i in range(len(ts)):          # ascending row order: later rows win
        last[seg_of[i], first[i]:end[i]] = vals[i]
    count = np.where(cnt > 0, cnt.astype(np.float64), NAN)
    return count, last


# -------------------------------------------------------------- series_last
EMPTY_TS = -(1 << 63) + 1


def series_last(sources, slot_lut, ts_lo, ts_hi, n_slots):
    """Per slot the lexicographic max of (ts, source index, row)."""
    best = [None] * n_slots
    for si, (ts, series) in enumerate(sources):
        for i in range(len(ts)):
            t, s = int(ts[i]), int(series[i])
            if not (ts_lo <= t < ts_hi) or not (0 <= s < len(slot_lut)):
                continue
            slot = int(slot_lut[s])
            if slot < 0:
                continue
            key = (t, si, i)
            if best[slot] is None or key > best[slot]:
                best[slot] = key
    out = np.array([b if b is not None else (EMPTY_TS, -1, -1) for b in best],
                   dtype=np.int64).reshape(n_slots, 3)
    return out[:, 0], out[:, 1], out[:, 2]


# ------------------------------------------------- filter / dedup / scatter
def filter_series_time(ts, series, slot_lut, ts_lo, ts_hi):
    keep = (ts >= ts_lo) & (ts < ts_hi)
    if slot_lut is not None:
        lut = np.asarray(slot_lut)
        inside = (series >= 0) & (series < len(lut))
        hit = np.zeros(len(ts), dtype=bool)
        hit[inside] = lut[series[inside]] >= 0
        keep &= hit
    return keep


def dedup_mark_last(series, ts):
    n = len(ts)
    keep = np.ones(n, dtype=bool)
    if n > 1:
        keep[:-1] = (series[:-1] != series[1:]) | (ts[:-1] != ts[1:])
    return keep


def scatter_append(ts, series, fields, region_of, dst_off, dst_ts, dst_se,
                   dst_fields):
    """Row loop into numpy destination arrays (modified in place)."""
    for i in range(len(ts)):
        r, o = int(region_of[i]), int(dst_off[i])
        dst_ts[r][o] = ts[i]
        dst_se[r][o] = series[i]
        dst_fields[r][:, o] = fields[:, i]


# --------------------------------------------------------------- RLE expand
def rle_expand(runs, blob, bw, n, only=None):
    """Hybrid RLE / bit-packed run table → values, by shifting one Python
    int that holds the whole blob (little-endian bit order). `only` limits
    the work to some output indices (the rest stay -1)."""
    big = int.from_bytes(bytes(blob), "little")
    mask = (1 << bw) - 1
    out = np.full(n, -1, dtype=np.int64)
    want = None if only is None else set(int(i) for i in only)
    for is_packed, off, val, start, count in (map(int, r) for r in runs):
        if want is None:
            js = range(count)
        else:
            js = [i - start for i in want if start <= i < start + count]
        for j in js:
            if is_packed:
                out[start + j] = (big >> (8 * off + j * bw)) & mask
            else:
                out[start + j] = val
    return out
