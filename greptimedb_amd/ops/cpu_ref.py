"""CPU reference implementations of the HIP kernels (plain PyTorch, fp64).

These define the semantics the gfx950 kernels in csrc/kernels.hip must match;
GPU numerics tests (tests/test_ops_gpu.py) compare the two. They also serve
as the execution path on CPU-only hosts (tests, CI).
"""

from __future__ import annotations

import torch


def ts_bucket_agg(ts, series, fields, field_idx, slot_lut, ts_lo, ts_hi,
                  origin, bucket_ms, n_slots, n_buckets):
    """Fused filter + time-bucket aggregate.

    ts: i64[n] ms, series: i32[n], fields: f64[nf_total, >=n],
    field_idx: i32[nf], slot_lut: i32[lut]. Returns (sum, count, min, max,
    rows) — the first four [nf, n_slots, n_buckets] (min/max NaN where
    count==0), rows [n_slots, n_buckets] = matching row count per cell
    (for count(*)/group existence). NaN field values are nulls, skipped.
    """
    n = ts.numel()
    keep = (ts >= ts_lo) & (ts < ts_hi)
    s = series.long().clamp(0, max(slot_lut.numel() - 1, 0))
    in_lut = (series >= 0) & (series < slot_lut.numel())
    slot = torch.where(in_lut, slot_lut[s].long(), torch.full_like(s, -1))
    keep &= slot >= 0
    bucket = torch.div(ts - origin, bucket_ms, rounding_mode="floor")
    keep &= (bucket >= 0) & (bucket < n_buckets)

    nf = field_idx.numel()
    out_sum = torch.zeros(nf, n_slots, n_buckets, dtype=torch.float64)
    out_cnt = torch.zeros(nf, n_slots, n_buckets, dtype=torch.int64)
    out_min = torch.full((nf, n_slots, n_buckets), float("nan"), dtype=torch.float64)
    out_max = torch.full((nf, n_slots, n_buckets), float("nan"), dtype=torch.float64)
    out_rows = torch.zeros(n_slots, n_buckets, dtype=torch.int64)

    idx = keep.nonzero(as_tuple=True)[0]
    if idx.numel() == 0:
        return out_sum, out_cnt, out_min, out_max, out_rows
    cell = slot[idx] * n_buckets + bucket[idx]
    out_rows.view(-1).index_add_(0, cell, torch.ones_like(cell))
    for f in range(nf):
        v = fields[int(field_idx[f])][:n][idx]
        ok = ~torch.isnan(v)
        c = cell[ok]
        vv = v[ok]
        out_sum[f].view(-1).index_add_(0, c, vv)
        out_cnt[f].view(-1).index_add_(0, c, torch.ones_like(c))
        mn = out_min[f].view(-1)
        mx = out_max[f].view(-1)
        mn.index_reduce_(0, c, vv, "amin", include_self=False)
        mx.index_reduce_(0, c, vv, "amax", include_self=False)
    # index_reduce with include_self=False leaves untouched cells at init NaN
    return out_sum, out_cnt, out_min, out_max, out_rows


def bucket_cells(ts, series, slot_lut, ts_lo, ts_hi, origin, bucket_ms,
                 n_buckets):
    """Cell id per row: slot * n_buckets + bucket as ts_bucket_agg assigns
    it, -1 where the row is filtered out. Returns i32[n]."""
    keep = (ts >= ts_lo) & (ts < ts_hi)
    s = series.long().clamp(0, max(slot_lut.numel() - 1, 0))
    in_lut = (series >= 0) & (series < slot_lut.numel())
    slot = torch.where(in_lut, slot_lut[s].long() if slot_lut.numel()
                       else torch.full_like(s, -1), torch.full_like(s, -1))
    bucket = torch.div(ts - origin, bucket_ms, rounding_mode="floor")
    keep &= (slot >= 0) & (bucket >= 0) & (bucket < n_buckets)
    cell = slot * n_buckets + bucket
    return torch.where(keep, cell, torch.full_like(cell, -1)).to(torch.int32)


MAX_QUANTILE_CELLS = 262144   # Q * n_cells the device histogram allows


def grouped_quantile(sources, field_of_sel, p_of_sel, n_cells, on_pass=None):
    """Exact grouped order statistics. sources: [(cell i32[n], fields
    f64[nf_total, >=n], field_idx i32[nf])] accumulate into one state;
    selection s reads field row field_idx[field_of_sel[s]] with p_of_sel[s].
    Returns (lo, hi f64[Q, n_cells], cnt i64[Q, n_cells]): per cell the
    non-NaN count, the value of rank k1 = floor((cnt-1)*p) and of rank
    min(k1+1, cnt-1); NaN where cnt == 0. Rows with cell < 0 are skipped."""
    import numpy as np
    Q = len(field_of_sel)
    if Q < 1 or len(p_of_sel) != Q:
        raise ValueError("grouped_quantile: one p per selection, at least one")
    if n_cells < 1 or Q * n_cells > MAX_QUANTILE_CELLS:
        raise RuntimeError(f"grouped_quantile: Q * n_cells = {Q} * {n_cells} "
                           f"exceeds {MAX_QUANTILE_CELLS}")
    if sum(int(c.numel()) for c, _f, _i in sources) >= 1 << 32:
        raise RuntimeError("grouped_quantile: rows overflow the u32 bins")
    lo = np.full((Q, n_cells), np.nan)
    hi = np.full((Q, n_cells), np.nan)
    cnt = np.zeros((Q, n_cells), dtype=np.int64)
    for s in range(Q):
        p = float(p_of_sel[s])
        if not 0.0 <= p <= 1.0:
            raise RuntimeError(f"p must lie in [0, 1], got {p}")
        cells, vals = [], []
        for cell, fields, fidx in sources:
            m = int(cell.numel())
            if m == 0:
                continue
            cells.append(cell.numpy())
            vals.append(fields[int(fidx[field_of_sel[s]])][:m].numpy())
        if not cells:
            continue
        c = np.concatenate(cells)
        v = np.concatenate(vals)
        ok = (c >= 0) & (c < n_cells) & ~np.isnan(v)
        c, v = c[ok], v[ok]
        order = np.argsort(c, kind="stable")
        c, v = c[order], v[order]
        ends = np.searchsorted(c, np.arange(n_cells), side="right")
        start = 0
        for ci in range(n_cells):
            end = int(ends[ci])
            if end > start:
                a = np.sort(v[start:end])
                m = end - start
                k1 = int(np.floor((m - 1) * p))
                cnt[s, ci] = m
                lo[s, ci] = a[k1]
                hi[s, ci] = a[min(k1 + 1, m - 1)]
            start = end
        if on_pass is not None:
            on_pass()
    return torch.from_numpy(lo), torch.from_numpy(hi), torch.from_numpy(cnt)


def quantile_lerp(lo, hi, cnt, p):
    """Final quantile from grouped_quantile's planes (numpy [Q, n_cells],
    p: [Q]): linear interpolation between ranks k1 and k1+1 with weight
    g = (cnt-1)*p - k1, in the two-sided form np.quantile uses so the result
    equals np.quantile(values, p) bit for bit. NaN where cnt == 0."""
    import numpy as np
    lo = np.asarray(lo, dtype=np.float64)
    hi = np.asarray(hi, dtype=np.float64)
    cnt = np.asarray(cnt, dtype=np.int64)
    pcol = np.asarray(p, dtype=np.float64).reshape(-1, *([1] * (lo.ndim - 1)))
    virt = np.maximum(cnt - 1, 0).astype(np.float64) * pcol
    g = virt - np.floor(virt)
    with np.errstate(invalid="ignore"):
        d = hi - lo
        out = lo + d * g
        upper = hi - d * (1.0 - g)
    out = np.where(g >= 0.5, upper, out)
    return np.where(cnt > 0, out, np.nan)


def pair_moments(x, y):
    """Two-pass second moments of paired float64 arrays without NaN →
    (n, mean_x, mean_y, m2x, m2y, cxy, const_x, const_y). m2 = Σ(x−x̄)²,
    cxy = Σ(x−x̄)(y−ȳ). A column is constant when min == max; its mean is
    then the value itself and its m2 (and cxy) exactly 0. n == 0: NaN means,
    zero sums, flags clear."""
    import numpy as np
    n = len(x)
    if n == 0:
        return 0, np.nan, np.nan, 0.0, 0.0, 0.0, False, False
    cx = bool(x.min() == x.max())
    cy = bool(y.min() == y.max())
    mx = float(x[0]) if cx else float(x.sum() / n)
    my = float(y[0]) if cy else float(y.sum() / n)
    with np.errstate(invalid="ignore"):
        dx = x - mx
        dy = y - my
        m2x = 0.0 if cx else float((dx * dx).sum())
        m2y = 0.0 if cy else float((dy * dy).sum())
        cxy = 0.0 if (cx or cy) else float((dx * dy).sum())
    return n, mx + 0.0, my + 0.0, m2x, m2y, cxy, cx, cy


def grouped_moments(sources, fx_of_sel, fy_of_sel, n_cells):
    """Grouped second moments. sources as for grouped_quantile; selection s
    pairs field rows field_idx[fx_of_sel[s]] and field_idx[fy_of_sel[s]]
    (fx == fy is the one-argument form). A row counts in its cell where the
    cell id lies in [0, n_cells) and neither value is NaN. Returns, each
    [M, n_cells]: n i64, mean_x, mean_y, m2x, m2y, cxy f64, const_x, const_y
    bool, per cell as pair_moments defines them."""
    import numpy as np
    M = len(fx_of_sel)
    if M < 1 or len(fy_of_sel) != M:
        raise ValueError("grouped_moments: one (x, y) pair per selection, at least one")
    if n_cells < 1 or M * n_cells > MAX_QUANTILE_CELLS:
        raise RuntimeError(f"grouped_moments: M * n_cells = {M} * {n_cells} "
                           f"exceeds {MAX_QUANTILE_CELLS}")
    for _c, _f, fidx in sources:
        for f in list(fx_of_sel) + list(fy_of_sel):
            if not 0 <= int(f) < int(fidx.numel()):
                raise RuntimeError(f"grouped_moments: selection field {f} "
                                   f"outside field_idx of length {fidx.numel()}")
    cnt = np.zeros((M, n_cells), dtype=np.int64)
    mean = np.full((2, M, n_cells), np.nan)
    acc = np.zeros((3, M, n_cells))
    const = np.zeros((2, M, n_cells), dtype=bool)
    for s in range(M):
        cells, xs, ys = [], [], []
        for cell, fields, fidx in sources:
            m = int(cell.numel())
            if m == 0:
                continue
            cells.append(cell.numpy())
            xs.append(fields[int(fidx[fx_of_sel[s]])][:m].numpy())
            ys.append(fields[int(fidx[fy_of_sel[s]])][:m].numpy())
        if not cells:
            continue
        c = np.concatenate(cells)
        x = np.concatenate(xs)
        y = np.concatenate(ys)
        ok = (c >= 0) & (c < n_cells) & ~np.isnan(x) & ~np.isnan(y)
        c, x, y = c[ok], x[ok], y[ok]
        order = np.argsort(c, kind="stable")
        c, x, y = c[order], x[order], y[order]
        ids, starts = np.unique(c, return_index=True)
        ends = np.append(starts[1:], len(c))
        for ci, a, b in zip(ids.tolist(), starts.tolist(), ends.tolist()):
            (cnt[s, ci], mean[0, s, ci], mean[1, s, ci], acc[0, s, ci],
             acc[1, s, ci], acc[2, s, ci], const[0, s, ci],
             const[1, s, ci]) = pair_moments(x[a:b], y[a:b])
    t = torch.from_numpy
    return (t(cnt), t(mean[0]), t(mean[1]), t(acc[0]), t(acc[1]), t(acc[2]),
            t(const[0]), t(const[1]))


MOMENT_KINDS = {"var_pop": 1, "var_samp": 1, "stddev_pop": 1, "stddev_samp": 1,
                "covar_pop": 2, "covar_samp": 2, "covar": 2, "corr": 2}


def moments_finish(kind, planes):
    """Final SQL value of moment aggregate `kind` from grouped_moments'
    planes (numpy arrays of any common shape) → (values f64, null bool).
      var_pop, stddev_pop  M2x/n, sqrt           NULL when n = 0
      var_samp, stddev_samp  M2x/(n−1), sqrt     NULL when n < 2
      covar_pop            C/n                   NULL when n = 0
      covar_samp, covar    C/(n−1)               NULL when n < 2
      corr                 C/sqrt(M2x·M2y) clamped to [−1, 1]; NULL when
                           n < 2 or x or y is constant (PostgreSQL's rule)
    Values are NaN where null."""
    import numpy as np
    n, _mx, _my, m2x, m2y, cxy, cx, cy = [np.asarray(p) for p in planes]
    if kind not in MOMENT_KINDS:
        raise ValueError(f"unknown moment aggregate {kind}")
    nf = n.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind in ("var_pop", "stddev_pop", "covar_pop"):
            null = n == 0
            out = (cxy if kind == "covar_pop" else m2x) / nf
        elif kind == "corr":
            null = (n < 2) | cx | cy
            out = np.clip(cxy / np.sqrt(m2x * m2y), -1.0, 1.0)
        else:
            null = n < 2
            out = (cxy if kind in ("covar_samp", "covar") else m2x) / (nf - 1.0)
        if kind.startswith("stddev"):
            out = np.sqrt(out)
    return np.where(null, np.nan, out), null


def filter_series_time(ts, series, slot_lut, ts_lo, ts_hi):
    keep = (ts >= ts_lo) & (ts < ts_hi)
    if slot_lut is not None and slot_lut.numel() > 0:
        in_lut = (series >= 0) & (series < slot_lut.numel())
        s = series.long().clamp(0, slot_lut.numel() - 1)
        keep &= in_lut & (slot_lut[s] >= 0)
    return keep


def series_last(sources, slot_lut, ts_lo, ts_hi, n_slots):
    """Lastpoint primitive: over sources [(ts, series), ...] (in recency
    order), find per slot the newest ts and its (source, row); later sources
    / later rows win ties. Returns (best_ts i64[n_slots], best_src i64,
    best_row i64), src/row = -1 where empty."""
    best_ts = torch.full((n_slots,), -(1 << 63) + 1, dtype=torch.int64)
    best_src = torch.full((n_slots,), -1, dtype=torch.int64)
    best_row = torch.full((n_slots,), -1, dtype=torch.int64)
    lut = slot_lut.long()
    for ts, series in sources:
        keep = (ts >= ts_lo) & (ts < ts_hi) & (series >= 0) & (series < lut.numel())
        idx = keep.nonzero(as_tuple=True)[0]
        if idx.numel() == 0:
            continue
        slots = lut[series.long()[idx]]
        ok = slots >= 0
        idx, slots = idx[ok], slots[ok]
        t = ts[idx]
        mx = torch.full((n_slots,), -(1 << 63) + 1, dtype=torch.int64)
        mx.index_reduce_(0, slots, t, "amax", include_self=True)
        best_ts = torch.maximum(best_ts, mx)
    best_pack = torch.full((n_slots,), -1, dtype=torch.int64)
    for si, (ts, series) in enumerate(sources):
        keep = (ts >= ts_lo) & (ts < ts_hi) & (series >= 0) & (series < lut.numel())
        idx = keep.nonzero(as_tuple=True)[0]
        if idx.numel() == 0:
            continue
        slots = lut[series.long()[idx]]
        ok = slots >= 0
        idx, slots = idx[ok], slots[ok]
        at = best_ts[slots] == ts[idx]
        ridx = at.nonzero(as_tuple=True)[0]
        # deterministic tie-break: max (source, row) wins (LastRow recency)
        pack = (si << 40) | idx[ridx]
        mx2 = torch.full((n_slots,), -1, dtype=torch.int64)
        mx2.index_reduce_(0, slots[ridx], pack, "amax", include_self=True)
        best_pack = torch.maximum(best_pack, mx2)
    found = best_pack >= 0
    best_src = torch.where(found, best_pack >> 40, best_src)
    best_row = torch.where(found, best_pack & ((1 << 40) - 1), best_row)
    return best_ts, best_src, best_row


PROM_MODES = {
    "instant": 0, "rate": 1, "increase": 2, "delta": 3,
    "avg_over_time": 4, "sum_over_time": 5, "min_over_time": 6,
    "max_over_time": 7, "count_over_time": 8, "last_over_time": 9,
    "idelta": 10, "irate": 11, "deriv": 12, "predict_linear": 13,
    "resets": 14, "changes": 15, "stddev_over_time": 16, "stdvar_over_time": 17,
    "absent_over_time": 18, "quantile_over_time": 19, "last_ts": 20,
}


def prom_range_eval(ts, vals, seg_lo, seg_hi, T, t0, step_ms, range_ms,
                    offset_ms, param, mode):
    """Reference implementation of the PromQL window evaluator (see
    csrc/kernels.hip prom_range_eval_kernel; semantics follow Prometheus'
    extrapolatedRate & friends)."""
    import numpy as np
    ts_h = ts.numpy() if torch.is_tensor(ts) else ts
    v_h = vals.numpy() if torch.is_tensor(vals) else vals
    lo_h = seg_lo.numpy() if torch.is_tensor(seg_lo) else seg_lo
    hi_h = seg_hi.numpy() if torch.is_tensor(seg_hi) else seg_hi
    S = len(lo_h)
    out = np.full((S, T), np.nan)
    for s in range(S):
        a0, b0 = int(lo_h[s]), int(hi_h[s])
        tseg = ts_h[a0:b0]
        vseg = v_h[a0:b0]
        for t in range(T):
            te = t0 + t * step_ms - offset_ms
            tb = te - range_ms
            w_lo = int(np.searchsorted(tseg, tb, "right"))
            w_hi = int(np.searchsorted(tseg, te, "right"))
            cnt = w_hi - w_lo
            w = vseg[w_lo:w_hi]
            wt = tseg[w_lo:w_hi]
            r = np.nan
            if mode in (0, 9):
                if cnt:
                    r = w[-1]
            elif mode == 20:       # last sample ts (dist last_value merge)
                if cnt:
                    r = float(wt[-1])
            elif mode == 8:
                if cnt:
                    r = float(cnt)
            elif mode == 18:
                r = np.nan if cnt else 1.0
            elif mode in (4, 5, 6, 7, 16, 17) and cnt:
                if mode == 5:
                    r = w.sum()
                elif mode == 4:
                    r = w.mean()
                elif mode == 6:
                    # Prometheus min/max_over_time skip NaN samples; the
                    # result is NaN only when every sample is NaN
                    r = np.fmin.reduce(w)
                elif mode == 7:
                    r = np.fmax.reduce(w)
                else:
                    var = ((w - w.mean()) ** 2).mean()
                    r = var if mode == 17 else np.sqrt(var)
            elif mode in (1, 2, 3) and cnt >= 2:
                is_counter = mode != 3
                total = w[-1] - w[0]
                if is_counter:
                    drops = np.diff(w)
                    if (drops < 0).any():
                        total += w[:-1][drops < 0].sum()
                sampled = (wt[-1] - wt[0]) / 1000.0
                range_s = range_ms / 1000.0
                avg_dur = sampled / (cnt - 1)
                dur_start = (wt[0] - tb) / 1000.0
                dur_end = (te - wt[-1]) / 1000.0
                if is_counter and total > 0 and w[0] >= 0:
                    dz = sampled * (w[0] / total)
                    dur_start = min(dur_start, dz)
                thresh = avg_dur * 1.1
                ext = sampled
                ext += dur_start if dur_start < thresh else avg_dur / 2
                ext += dur_end if dur_end < thresh else avg_dur / 2
                factor = ext / sampled if sampled > 0 else 1.0
                r = total * factor
                if mode == 1:
                    r /= range_s
            elif mode in (10, 11) and cnt >= 2:
                dv = w[-1] - w[-2]
                dt = (wt[-1] - wt[-2]) / 1000.0
                if mode == 10:
                    r = dv
                else:
                    d = w[-1] if w[-1] < w[-2] else dv
                    r = d / dt if dt > 0 else np.nan
            elif mode in (12, 13) and cnt >= 2:
                x = (wt - te) / 1000.0
                n = float(cnt)
                sx, sy = x.sum(), w.sum()
                sxx, sxy = (x * x).sum(), (x * w).sum()
                den = n * sxx - sx * sx
                if den != 0:
                    slope = (n * sxy - sx * sy) / den
                    intercept = (sy - slope * sx) / n
                    r = slope if mode == 12 else intercept + slope * param
            elif mode in (14, 15) and cnt >= 1:
                d = np.diff(w)
                r = float((d < 0).sum()) if mode == 14 else float((d != 0).sum())
            elif mode == 19 and cnt:
                # Prometheus quantile: sorted linear interpolation; q outside
                # [0,1] yields ∓Inf (promql/quantile.go)
                if param < 0:
                    r = -np.inf
                elif param > 1:
                    r = np.inf
                else:
                    sw = np.sort(w)
                    rank = param * (cnt - 1)
                    lo_i = int(np.floor(rank))
                    hi_i = min(lo_i + 1, cnt - 1)
                    r = sw[lo_i] + (sw[hi_i] - sw[lo_i]) * (rank - lo_i)
            out[s, t] = r
    return torch.as_tensor(out)


def dedup_mark_last(series, ts):
    """keep[i] ⇔ row i is the last of its (series, ts) group (sorted input)."""
    n = ts.numel()
    if n == 0:
        return torch.zeros(0, dtype=torch.bool)
    keep = torch.ones(n, dtype=torch.bool)
    keep[:-1] = (series[:-1] != series[1:]) | (ts[:-1] != ts[1:])
    return keep


def merge_last_non_null(series, ts, fields):
    """last_non_null merge over (series, ts, seq)-sorted rows →
    (kidx i64[g], merged f64[nf, g]). kidx are the group-last rows
    (dedup_mark_last(...).nonzero()); merged[f, j] is the value of the
    highest row of group j whose fields[f] is not NaN (NaN = NULL), or the
    group-last row's own bits when the whole group is NaN.

    A running maximum of "row index where valid, group start - 1 where not"
    gives every row the newest valid row at or before it; group starts only
    grow, so a value carried in from an earlier group is always below the
    current group's start and reads as "none"."""
    n = ts.numel()
    nf = fields.shape[0]
    if n == 0:
        return (torch.zeros(0, dtype=torch.int64),
                torch.zeros((nf, 0), dtype=torch.float64))
    kidx = dedup_mark_last(series, ts).nonzero(as_tuple=True)[0]
    g = kidx.numel()
    start = torch.zeros(g, dtype=torch.int64)
    start[1:] = kidx[:-1] + 1
    row_start = torch.repeat_interleave(start, kidx - start + 1)   # [n]
    rows = torch.arange(n, dtype=torch.int64)
    merged = torch.empty((nf, g), dtype=torch.float64)
    for f in range(nf):
        col = fields[f]
        cand = torch.where(torch.isnan(col), row_start - 1, rows)
        newest = torch.cummax(cand, 0).values[kidx]
        merged[f] = col[torch.where(newest >= start, newest, kidx)]
    return kidx, merged


def gorilla_encode(ts, vals, block, pack_ts=True):
    """Oracle for kernels.gorilla_encode (K20): gorilla.pack is the
    specification. → (blob u8, block_off i64[B], out_off i64[B], n);
    `vals` None packs like a column of zeros."""
    import numpy as np
    from greptimedb_amd.engine import gorilla
    ts_h = ts.numpy()
    v_h = np.zeros(len(ts_h)) if vals is None else vals.numpy()
    blob, block_off, out_off, n = gorilla.pack(ts_h, v_h, block,
                                               pack_ts=pack_ts)
    return (torch.as_tensor(np.frombuffer(blob, dtype=np.uint8).copy()),
            torch.as_tensor(block_off), torch.as_tensor(out_off), n)


def scatter_append(ts, series, fields, region_of, dst_off,
                   dst_ts, dst_se, dst_fields):
    """Oracle for kernels.scatter_append (K16): routed bulk memtable write."""
    for r in range(len(dst_ts)):
        m = region_of == r
        if not bool(m.any()):
            continue
        o = dst_off[m]
        dst_ts[r][o] = ts[m]
        dst_se[r][o] = series[m]
        dst_fields[r][:, o] = fields[:, m]


def packed_segments(stage, n, nf):
    """Views (ts i64[n], fields f64[nf, n], dst_off i64[n], series i32[n],
    region i32[n]) into a packed stage block — a uint8 CPU tensor laid out
    as csrc/ingest_core.h StageLayout (8-byte aligned segments)."""
    pad4 = (4 * n + 7) & ~7
    o_f = 8 * n
    o_d = o_f + 8 * nf * n
    o_s = o_d + 8 * n
    o_r = o_s + pad4
    ts = stage[:o_f].view(torch.int64)
    fields = stage[o_f:o_d].view(torch.float64).reshape(nf, n)
    dst_off = stage[o_d:o_s].view(torch.int64)
    series = stage[o_s:o_s + 4 * n].view(torch.int32)
    region = stage[o_r:o_r + 4 * n].view(torch.int32)
    return ts, fields, dst_off, series, region


def scatter_append_packed(stage_host, stage_dev, n, nf, bases,
                          dst_ts, dst_se, dst_fields):
    """Oracle for kernels.scatter_append_packed: row i of the packed block
    goes to region region[i] at row bases[region[i]] + dst_off[i]. On CPU
    there is no upload, so `stage_dev` is unused."""
    if n == 0:
        return
    ts, fields, dst_off, series, region = packed_segments(stage_host, n, nf)
    dst = dst_off + torch.as_tensor(list(bases), dtype=torch.int64)[region.long()]
    scatter_append(ts, series, fields, region, dst, dst_ts, dst_se,
                   [f[:nf] for f in dst_fields])
