// CDNA4 (gfx950 / MI355X) kernels for the mito-hip scan, ingest and cold-tier
// paths. Launchers are declared in kernels.h and defined at the end of this
// file; csrc/hip_ops.cpp binds them to torch.
//
// Kernel inventory (SURVEY.md §2.7 numbering), in file order:
//  - decode_minmax_kernel : K5 finish, min/max order keys -> f64.
//  - filter_series_time_kernel : K1/K2 keep-mask for raw scans.
//  - dedup_mark_last_kernel : K4 last_row marker on (series, ts)-sorted data.
//  - merge_last_non_null_kernel : K4 last_non_null merge, per field the newest
//    non-NULL value of each (series, ts) group.
//  - bucket_cell_coalesced_kernel + field_bucket_agg_lds_kernel : fused K1
//    (predicate filter via series LUT) + K2 (time-range visibility) + K5
//    (time-bucket aggregate): sum/count/min/max of every requested field
//    into [nf, n_slots, n_buckets] accumulators, in LDS-privatized tiles.
//  - series_last_ts_kernel / series_last_row_kernel : lastpoint, per-slot
//    argmax(ts) with a (source, row) tie-break.
//  - prom_range_eval_kernel : K7/K8 PromQL selector and range functions.
//  - quantile_{hist,pick,next,finish}_kernel : K21 exact grouped order
//    statistics by radix-histogram selection over bucket cells.
//  - moments_{sums,mean,centred}_kernel : K22 grouped second moments
//    (variance, covariance, correlation) in two passes over bucket cells.
//  - scatter_append_kernel / scatter_append_packed_kernel : K16 routed
//    ingest batch -> region memtables.
//  - rle_expand_indices_kernel : K11 parquet hybrid RLE/bit-packed indices.
//  - gorilla_decode_kernel / gorilla_{scale,widths,write}_kernel : K20 cold
//    tier, fixed-width-per-block delta codec, decoded and encoded in HBM.
//
// Design notes (cdna_hip_programming.md):
//  * 256-thread blocks (4 waves of 64), grid-stride, grid capped at
//    2048 blocks (G11: memory-bound ops).
//  * f64 min/max accumulate through the monotonic u64 key mapping so we can
//    use hardware atomicMin/Max on unsigned long long (no f64 min/max atomic).
//  * NaN field values are nulls (influx missing fields) and are skipped.
//  * Accumulators with many writers per address are privatized in LDS per
//    row tile (bucket aggregate, quantile histograms) and flushed once per
//    tile; a tile whose cells do not fit the LDS table uses global atomics.

#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"

#define DEV_INLINE __device__ __forceinline__

namespace gdb_hip {

// IEEE-754 double <-> totally-ordered u64 (sign-flip transform): key order ==
// numeric order, so u64 atomicMin/Max order doubles and order statistics can
// be selected bitwise.
DEV_INLINE uint64_t f64_to_key(double d) {
  uint64_t bits = __double_as_longlong(d);
  return (int64_t)bits < 0 ? ~bits : (bits | 0x8000000000000000ULL);
}

DEV_INLINE double key_to_f64(uint64_t key) {
  uint64_t bits = (key & 0x8000000000000000ULL) ? (key & 0x7FFFFFFFFFFFFFFFULL) : ~key;
  return __longlong_as_double(bits);
}

DEV_INLINE double quiet_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// Bucket index = floor((t - origin) / bucket_ms), as cpu_ref defines it.
// C++ '/' truncates toward zero, which would fold origin-bucket_ms < t <
// origin into bucket 0; every t < origin floors below 0 (bucket_ms > 0), so
// it maps to -1 and callers drop it with their b < 0 test.
DEV_INLINE int64_t bucket_index(int64_t t, int64_t origin, int64_t bucket_ms) {
  const int64_t d = t - origin;
  return d < 0 ? -1 : d / bucket_ms;
}

// Row visibility (K1 + K2): whether row i, with timestamp t, is visible, and
// if so its slot. Not visible: t outside [ts_lo, ts_hi), series[i] outside
// the LUT (an empty LUT hides every row), or a negative LUT entry. series[i]
// is read only for a row inside the time window. Only a caller whose contract
// says so passes null_lut_is_all: a null slot_lut then selects every series
// (slot 0) without reading series at all.
// A bool with the slot on the side, not "slot or -1": the callers' early
// `continue`s then compile to the branches they were when written out.
DEV_INLINE bool visible_row(int64_t t, const int32_t* __restrict__ series,
                            int64_t i, const int32_t* __restrict__ slot_lut,
                            int lut_size, int64_t ts_lo, int64_t ts_hi,
                            int32_t& slot, bool null_lut_is_all = false) {
  slot = 0;
  if (t < ts_lo || t >= ts_hi) return false;
  if (null_lut_is_all && slot_lut == nullptr) return true;
  const int32_t s = series[i];
  if (s < 0 || s >= lut_size) return false;
  slot = slot_lut[s];
  return slot >= 0;
}

// ------------------------------------------------------------- K5 finish
// decode min/max key arrays into f64 (count==0 → NaN)
__global__ void decode_minmax_kernel(
    const unsigned long long* __restrict__ minkey,
    const unsigned long long* __restrict__ maxkey,
    const unsigned long long* __restrict__ cnt,
    double* __restrict__ out_min, double* __restrict__ out_max, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (cnt[i] == 0) {
      out_min[i] = quiet_nan();
      out_max[i] = quiet_nan();
    } else {
      out_min[i] = key_to_f64(minkey[i]);
      out_max[i] = key_to_f64(maxkey[i]);
    }
  }
}

// ---------------------------------------------------------------- K1/K2 mask
__global__ void filter_series_time_kernel(
    const int64_t* __restrict__ ts,
    const int32_t* __restrict__ series,
    const int32_t* __restrict__ slot_lut, int lut_size,  // lut==nullptr → all series
    int64_t ts_lo, int64_t ts_hi, int64_t n,
    bool* __restrict__ keep) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int32_t slot;
    keep[i] = visible_row(ts[i], series, i, slot_lut, lut_size, ts_lo, ts_hi,
                          slot, /*null_lut_is_all=*/true);
  }
}

// ---------------------------------------------------------------- K4 dedup
// Input sorted ascending by (series, ts, seq). Keep the LAST row of each
// (series, ts) group (reference read/dedup.rs LastRow semantics).
__global__ void dedup_mark_last_kernel(
    const int32_t* __restrict__ series,
    const int64_t* __restrict__ ts,
    int64_t n, bool* __restrict__ keep) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    keep[i] = (i == n - 1) || (series[i] != series[i + 1]) || (ts[i] != ts[i + 1]);
  }
}

// ---------------------------------------------------------------- K4 merge
// last_non_null merge (reference read/dedup.rs LastNonNull): for group j of
// the (series, ts, seq)-sorted input and field f, the output is the value of
// the highest row of the group that is not NaN (NaN = NULL), or the group-last
// row's own bits when every row is NaN. kidx[j] is the last row of group j
// (the dedup_mark_last rows), so group j starts at kidx[j-1] + 1.
//
// Design: look-back, not a tile-level segmented scan. The output has one
// element per GROUP, and almost every group has one row, so the common case
// should read each kept element once and write it once: one lane per group
// (coalesced over j; kidx[j] grows by one per lane there, so the field read
// is coalesced too), the two kidx loads shared by all nf fields. A scan
// would carry a (value, flag) pair through LDS for every input row to serve
// the rare long group. A NULL last row first tries LNN_LOOKBACK earlier rows
// in its own lane (short groups: partial writes of a few fields). Whatever
// is still unresolved is taken over by the whole wave, one group at a time:
// 64 rows per step, newest first, the newest valid lane picked with a ballot,
// stopping at the group start. Every row of a group is read at most once per
// field, so the pass stays O(n * nf) however long a group is.
constexpr int LNN_LOOKBACK = 4;

__global__ void __launch_bounds__(256) merge_last_non_null_kernel(
    const int64_t* __restrict__ kidx, int64_t g,
    const double* __restrict__ fields, int64_t field_stride, int nf,
    double* __restrict__ out) {              // [nf, g]
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // the loop bound depends on the wave's first group only: all 64 lanes stay
  // in the loop together, which the ballots and shuffles below rely on
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane);
       base < g; base += stride) {
    const int64_t j = base + lane;
    const bool active = j < g;
    const int64_t last = active ? kidx[j] : 0;
    const int64_t start = (active && j > 0) ? kidx[j - 1] + 1 : 0;
    for (int f = 0; f < nf; f++) {
      const double* __restrict__ col = fields + (int64_t)f * field_stride;
      double v = 0.0;
      bool need = false;
      int64_t hi = -1;                       // next (older) row to examine
      if (active) {
        v = col[last];
        if (isnan(v) && last > start) {
          need = true;
          hi = last - 1;
          for (int k = 0; k < LNN_LOOKBACK && hi >= start; k++, hi--) {
            const double w = col[hi];
            if (!isnan(w)) { v = w; need = false; break; }
          }
          if (hi < start) need = false;      // group exhausted: keep the NaN
        }
      }
      unsigned long long todo = __ballot(need);
      while (todo) {
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1;
        const int64_t s_start = __shfl(start, src);
        const int64_t s_hi = __shfl(hi, src);
        double fv = 0.0;
        bool found = false;
        for (int64_t top = s_hi; top >= s_start; top -= 64) {
          const int64_t r = top - lane;      // lane 0 holds the newest row
          const bool in = r >= s_start;
          const double w = in ? col[r] : 0.0;
          const unsigned long long ok = __ballot(in && !isnan(w));
          if (ok) {
            fv = __shfl(w, __ffsll(ok) - 1);
            found = true;
            break;
          }
        }
        if (found && lane == src) v = fv;
      }
      if (active) out[(int64_t)f * g + j] = v;
    }
  }
}

// ---------------------------------------------------------------- K1+K2+K5
// Fused filter + time-bucket aggregate in two launches.
// bucket_cell_coalesced_kernel: one thread per row, coalesced, writes the
// row's (slot, bucket) cell id, slot * n_buckets + bucket, or -1 where the
// row is filtered out; every field reuses it.
// field_bucket_agg_lds_kernel: one block per tile of AGG_TILE rows, threads
// striding the tile contiguously so loads stay coalesced. Scan sources are
// (series, ts)-sorted, so a tile spans few cells: the accumulator table of
// the tile's cell range is privatized in LDS (per-element LDS atomics) and
// flushed to the global [nf, n_slots, n_buckets] accumulators once per tile
// and field. A tile whose cell range exceeds LDS_CELLS (unsorted input)
// falls back to global atomics, still with coalesced loads.
// fields: column-major per field: fields[f * field_stride + row]

__global__ void bucket_cell_coalesced_kernel(
    const int64_t* __restrict__ ts,
    const int32_t* __restrict__ series,
    const int32_t* __restrict__ slot_lut, int lut_size,
    int64_t ts_lo, int64_t ts_hi, int64_t origin, int64_t bucket_ms,
    int n_buckets, int64_t n,
    int32_t* __restrict__ cell) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t t = ts[i];
    int32_t slot, cl = -1;
    if (visible_row(t, series, i, slot_lut, lut_size, ts_lo, ts_hi, slot)) {
      const int64_t b = bucket_index(t, origin, bucket_ms);
      if (b >= 0 && b < n_buckets) cl = slot * n_buckets + (int32_t)b;
    }
    cell[i] = cl;
  }
}

__global__ void field_bucket_agg_lds_kernel(
    const int32_t* __restrict__ cell,
    const double* __restrict__ fields, int64_t field_stride,
    const int32_t* __restrict__ field_idx, int nf,
    int64_t n, int64_t cells_per_field,
    double* __restrict__ out_sum,
    unsigned long long* __restrict__ out_cnt,
    unsigned long long* __restrict__ out_min,
    unsigned long long* __restrict__ out_max,
    unsigned long long* __restrict__ out_rows) {
  __shared__ int32_t s_lo, s_hi;
  __shared__ double s_sum[LDS_CELLS];
  __shared__ unsigned long long s_cnt[LDS_CELLS];
  __shared__ unsigned long long s_min[LDS_CELLS];
  __shared__ unsigned long long s_max[LDS_CELLS];
  const int tid = threadIdx.x;
  const int nthreads = blockDim.x;
  const int64_t ntiles = (n + AGG_TILE - 1) / AGG_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t t0 = tile * AGG_TILE;
    const int64_t t1 = min(t0 + (int64_t)AGG_TILE, n);
    if (tid == 0) { s_lo = INT32_MAX; s_hi = -1; }
    __syncthreads();
    int32_t my_lo = INT32_MAX, my_hi = -1;
    for (int64_t i = t0 + tid; i < t1; i += nthreads) {
      const int32_t c = cell[i];
      if (c >= 0) { my_lo = min(my_lo, c); my_hi = max(my_hi, c); }
    }
    if (my_hi >= 0) {
      atomicMin(&s_lo, my_lo);
      atomicMax(&s_hi, my_hi);
    }
    __syncthreads();
    const int32_t lo = s_lo, hi = s_hi;
    __syncthreads();
    if (hi < 0) continue;                       // tile fully filtered out
    const int range = hi - lo + 1;
    if (range <= LDS_CELLS) {
      // rows count once per tile (reuse s_cnt as the rows table)
      for (int k = tid; k < range; k += nthreads) s_cnt[k] = 0ULL;
      __syncthreads();
      for (int64_t i = t0 + tid; i < t1; i += nthreads) {
        const int32_t c = cell[i];
        if (c >= 0) atomicAdd(&s_cnt[c - lo], 1ULL);
      }
      __syncthreads();
      for (int k = tid; k < range; k += nthreads)
        if (s_cnt[k]) atomicAdd(&out_rows[lo + k], s_cnt[k]);
      __syncthreads();
      for (int f = 0; f < nf; f++) {
        const double* __restrict__ col =
            fields + (int64_t)field_idx[f] * field_stride;
        for (int k = tid; k < range; k += nthreads) {
          s_sum[k] = 0.0; s_cnt[k] = 0ULL; s_min[k] = ~0ULL; s_max[k] = 0ULL;
        }
        __syncthreads();
        for (int64_t i = t0 + tid; i < t1; i += nthreads) {
          const int32_t c = cell[i];
          if (c < 0) continue;
          const double v = col[i];
          if (isnan(v)) continue;
          const int k = c - lo;
          atomicAdd(&s_sum[k], v);
          atomicAdd(&s_cnt[k], 1ULL);
          const uint64_t key = f64_to_key(v);
          atomicMin(&s_min[k], (unsigned long long)key);
          atomicMax(&s_max[k], (unsigned long long)key);
        }
        __syncthreads();
        const int64_t base = (int64_t)f * cells_per_field;
        for (int k = tid; k < range; k += nthreads) {
          if (!s_cnt[k]) continue;
          atomicAdd(&out_sum[base + lo + k], s_sum[k]);
          atomicAdd(&out_cnt[base + lo + k], s_cnt[k]);
          atomicMin(&out_min[base + lo + k], s_min[k]);
          atomicMax(&out_max[base + lo + k], s_max[k]);
        }
        __syncthreads();
      }
    } else {
      // wide tile (unsorted data): coalesced loads, global atomics
      for (int64_t i = t0 + tid; i < t1; i += nthreads) {
        const int32_t c = cell[i];
        if (c >= 0) atomicAdd(&out_rows[c], 1ULL);
      }
      for (int f = 0; f < nf; f++) {
        const double* __restrict__ col =
            fields + (int64_t)field_idx[f] * field_stride;
        const int64_t base = (int64_t)f * cells_per_field;
        for (int64_t i = t0 + tid; i < t1; i += nthreads) {
          const int32_t c = cell[i];
          if (c < 0) continue;
          const double v = col[i];
          if (isnan(v)) continue;
          atomicAdd(&out_sum[base + c], v);
          atomicAdd(&out_cnt[base + c], 1ULL);
          const uint64_t key = f64_to_key(v);
          atomicMin(&out_min[base + c], (unsigned long long)key);
          atomicMax(&out_max[base + c], (unsigned long long)key);
        }
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------- K-lastpoint (series last)
// Monotonic i64→u64 key so unsigned atomicMax orders signed timestamps.
DEV_INLINE uint64_t i64_to_key(int64_t v) {
  return (uint64_t)v ^ 0x8000000000000000ULL;
}

// pass 1: per-slot max ts (key-mapped); best init 0
__global__ void series_last_ts_kernel(
    const int64_t* __restrict__ ts,
    const int32_t* __restrict__ series,
    const int32_t* __restrict__ slot_lut, int lut_size,
    int64_t ts_lo, int64_t ts_hi, int64_t n,
    unsigned long long* __restrict__ best_key) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t t = ts[i];
    int32_t slot;
    if (!visible_row(t, series, i, slot_lut, lut_size, ts_lo, ts_hi, slot)) continue;
    atomicMax(&best_key[slot], (unsigned long long)i64_to_key(t));
  }
}

// pass 2: among rows whose ts matches the winner, pick (src_tag, row) max —
// later sources / later arrivals win ties (LastRow semantics)
__global__ void series_last_row_kernel(
    const int64_t* __restrict__ ts,
    const int32_t* __restrict__ series,
    const int32_t* __restrict__ slot_lut, int lut_size,
    int64_t ts_lo, int64_t ts_hi, int64_t n,
    const unsigned long long* __restrict__ best_key,
    unsigned long long src_tag,                    // source index (recency order)
    unsigned long long* __restrict__ best_row) {   // (src_tag<<40)|row ; init 0
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t t = ts[i];
    int32_t slot;
    if (!visible_row(t, series, i, slot_lut, lut_size, ts_lo, ts_hi, slot)) continue;
    if ((unsigned long long)i64_to_key(t) != best_key[slot]) continue;
    // +1 so "no row" (0) is distinguishable from src 0 row 0
    atomicMax(&best_row[slot], (src_tag << 40) | ((unsigned long long)i + 1));
  }
}

// ------------------------------------------------- K7/K8 PromQL evaluators
//
// One kernel evaluates a PromQL selector/range-function over a
// (slot, ts)-sorted sample array onto the query step grid. Thread =
// (slot, step): binary-search the window bounds inside the slot's segment,
// then reduce the window per `mode`. Rate/increase/delta follow Prometheus'
// extrapolation rules exactly (reference: promql/functions/extrapolate_rate.rs,
// itself a port of Prometheus' extrapolatedRate).

enum PromMode {
  PM_INSTANT = 0, PM_RATE = 1, PM_INCREASE = 2, PM_DELTA = 3,
  PM_AVG = 4, PM_SUM = 5, PM_MIN = 6, PM_MAX = 7, PM_COUNT = 8, PM_LAST = 9,
  PM_IDELTA = 10, PM_IRATE = 11, PM_DERIV = 12, PM_PREDICT = 13,
  PM_RESETS = 14, PM_CHANGES = 15, PM_STDDEV = 16, PM_STDVAR = 17,
  PM_ABSENT_OT = 18, PM_QUANTILE_OT = 19, PM_LAST_TS = 20,
};

__global__ void prom_range_eval_kernel(
    const int64_t* __restrict__ ts,
    const double* __restrict__ vals,
    const int64_t* __restrict__ seg_lo,   // [S] first row of slot
    const int64_t* __restrict__ seg_hi,   // [S] one past last row
    int S, int T,
    int64_t t0, int64_t step_ms, int64_t range_ms, int64_t offset_ms,
    double param, int mode,
    double* __restrict__ out) {           // [S, T]
  const int64_t total = (int64_t)S * T;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int s = (int)(i / T);
    const int t = (int)(i % T);
    const int64_t te = t0 + (int64_t)t * step_ms - offset_ms;   // window end (inclusive)
    const int64_t tb = te - range_ms;                           // window begin (exclusive)
    const int64_t lo = seg_lo[s], hi = seg_hi[s];
    // lower: first idx with ts > tb ; upper: last idx with ts <= te
    int64_t a = lo, b = hi;
    while (a < b) { int64_t m = (a + b) >> 1; if (ts[m] <= tb) a = m + 1; else b = m; }
    const int64_t w_lo = a;
    a = w_lo; b = hi;
    while (a < b) { int64_t m = (a + b) >> 1; if (ts[m] <= te) a = m + 1; else b = m; }
    const int64_t w_hi = a;                                     // exclusive
    const int64_t cnt = w_hi - w_lo;
    double r = quiet_nan();
    if (mode == PM_INSTANT) {
      if (cnt > 0) r = vals[w_hi - 1];
    } else if (mode == PM_LAST) {
      if (cnt > 0) r = vals[w_hi - 1];
    } else if (mode == PM_LAST_TS) {
      // last sample timestamp as f64 (exact to 2^53 ms) — the cross-rank
      // last_value merge argmaxes on this plane
      if (cnt > 0) r = (double)ts[w_hi - 1];
    } else if (mode == PM_COUNT) {
      if (cnt > 0) r = (double)cnt;
    } else if (mode == PM_ABSENT_OT) {
      r = (cnt > 0) ? quiet_nan() : 1.0;
    } else if (cnt > 0 && (mode == PM_SUM || mode == PM_AVG || mode == PM_MIN ||
                           mode == PM_MAX || mode == PM_STDDEV || mode == PM_STDVAR)) {
      double sum = 0, mn = vals[w_lo], mx = vals[w_lo];
      for (int64_t j = w_lo; j < w_hi; j++) {
        const double v = vals[j];
        sum += v; mn = fmin(mn, v); mx = fmax(mx, v);
      }
      if (mode == PM_SUM) r = sum;
      else if (mode == PM_AVG) r = sum / cnt;
      else if (mode == PM_MIN) r = mn;
      else if (mode == PM_MAX) r = mx;
      else {
        const double mean = sum / cnt;
        double aux = 0;
        for (int64_t j = w_lo; j < w_hi; j++) {
          const double d = vals[j] - mean;
          aux += d * d;
        }
        const double var = aux / cnt;
        r = (mode == PM_STDVAR) ? var : sqrt(var);
      }
    } else if (cnt >= 2 && (mode == PM_RATE || mode == PM_INCREASE || mode == PM_DELTA)) {
      const bool is_counter = (mode != PM_DELTA);
      const double first_v = vals[w_lo], last_v = vals[w_hi - 1];
      const int64_t first_t = ts[w_lo], last_t = ts[w_hi - 1];
      double total_incr = last_v - first_v;
      if (is_counter) {
        double prev = first_v;
        for (int64_t j = w_lo + 1; j < w_hi; j++) {
          const double v = vals[j];
          if (v < prev) total_incr += prev;   // counter reset correction
          prev = v;
        }
      }
      const double sampled = (double)(last_t - first_t) / 1000.0;
      const double range_s = (double)range_ms / 1000.0;
      const double avg_dur = sampled / (cnt - 1);
      double dur_to_start = (double)(first_t - tb) / 1000.0;
      const double dur_to_end = (double)(te - last_t) / 1000.0;
      if (is_counter && total_incr > 0 && first_v >= 0) {
        const double dur_to_zero = sampled * (first_v / total_incr);
        if (dur_to_zero < dur_to_start) dur_to_start = dur_to_zero;
      }
      const double thresh = avg_dur * 1.1;
      double ext = sampled;
      ext += (dur_to_start < thresh) ? dur_to_start : avg_dur / 2;
      ext += (dur_to_end < thresh) ? dur_to_end : avg_dur / 2;
      const double factor = (sampled > 0) ? ext / sampled : 1.0;
      double res = total_incr * factor;
      if (mode == PM_RATE) res /= range_s;
      r = res;
    } else if (cnt >= 2 && (mode == PM_IDELTA || mode == PM_IRATE)) {
      const double dv = vals[w_hi - 1] - vals[w_hi - 2];
      const double dt = (double)(ts[w_hi - 1] - ts[w_hi - 2]) / 1000.0;
      if (mode == PM_IDELTA) {
        r = dv;
      } else {
        double v2 = vals[w_hi - 1], v1 = vals[w_hi - 2];
        double d = (v2 < v1) ? v2 : dv;   // reset → use raw value
        r = (dt > 0) ? d / dt : quiet_nan();
      }
    } else if (cnt >= 2 && (mode == PM_DERIV || mode == PM_PREDICT)) {
      // least-squares slope/intercept, x relative to window end (Prometheus
      // uses intercept at `te`)
      double sx = 0, sy = 0, sxx = 0, sxy = 0;
      for (int64_t j = w_lo; j < w_hi; j++) {
        const double x = (double)(ts[j] - te) / 1000.0;
        const double y = vals[j];
        sx += x; sy += y; sxx += x * x; sxy += x * y;
      }
      const double nn = (double)cnt;
      const double den = nn * sxx - sx * sx;
      if (den != 0) {
        const double slope = (nn * sxy - sx * sy) / den;
        const double intercept = (sy - slope * sx) / nn;
        r = (mode == PM_DERIV) ? slope : intercept + slope * param;
      }
    } else if (cnt >= 1 && (mode == PM_RESETS || mode == PM_CHANGES)) {
      double prev = vals[w_lo];
      int64_t k = 0;
      for (int64_t j = w_lo + 1; j < w_hi; j++) {
        const double v = vals[j];
        if (mode == PM_RESETS ? (v < prev) : (v != prev)) k++;
        prev = v;
      }
      r = (double)k;
    } else if (cnt >= 1 && mode == PM_QUANTILE_OT) {
      // Prometheus quantile: sorted linear interpolation (promql/quantile.go);
      // q outside [0,1] yields ∓Inf. Small windows (the common case: ≤128
      // samples) insertion-sort in scratch; larger windows select the two
      // needed order statistics by O(W²) rank counting — no extra storage.
      const double q = param;
      if (q < 0.0) {
        r = -INFINITY;
      } else if (q > 1.0) {
        r = INFINITY;
      } else {
        const double rank = q * (double)(cnt - 1);
        const int64_t k1 = (int64_t)rank;
        const int64_t k2 = (k1 + 1 < cnt) ? k1 + 1 : k1;
        double vk1 = NAN, vk2 = NAN;
        if (cnt <= 128) {
          double buf[128];
          int64_t m = 0;
          for (int64_t j = w_lo; j < w_hi; j++) {
            const double v = vals[j];
            int64_t p = m++;
            while (p > 0 && buf[p - 1] > v) { buf[p] = buf[p - 1]; p--; }
            buf[p] = v;
          }
          vk1 = buf[k1];
          vk2 = buf[k2];
        } else {
          // radix bisection on the sort-key transform: O(64·W) instead of
          // the old O(W²) rank counting. Register-only on purpose — each
          // thread owns its WHOLE ragged window (windows ≫ threads per
          // launch), so cooperative LDS staging would idle the rest of the
          // wavefront; per-thread bitwise selection is the CDNA4-shaped
          // answer for this layout.
          uint64_t prefix = 0;
          int64_t k = k1;
          for (int bit = 63; bit >= 0; bit--) {
            const uint64_t high_mask =
                (bit == 63) ? 0ULL : (~0ULL << (bit + 1));
            const uint64_t b = 1ULL << bit;
            int64_t cnt0 = 0;
            for (int64_t j = w_lo; j < w_hi; j++) {
              const uint64_t kj = f64_to_key(vals[j]);
              cnt0 += ((kj & high_mask) == prefix) & !(kj & b);
            }
            if (k >= cnt0) { k -= cnt0; prefix |= b; }
          }
          const uint64_t kk = prefix;   // exact key of rank k1
          int64_t less = 0, eq = 0;
          uint64_t next = ~0ULL;
          bool has_next = false;
          for (int64_t j = w_lo; j < w_hi; j++) {
            const uint64_t kj = f64_to_key(vals[j]);
            if (kj < kk) less++;
            else if (kj == kk) eq++;
            else if (kj < next) { next = kj; has_next = true; }
          }
          vk1 = key_to_f64(kk);
          vk2 = (k2 < less + eq || !has_next) ? vk1 : key_to_f64(next);
        }
        r = vk1 + (vk2 - vk1) * (rank - (double)k1);
      }
    }
    out[i] = r;
  }
}

// ------------------------------------- K21 grouped radix-histogram selection
//
// Exact order statistics per (selection, cell) with no sort: a selection is
// a (field column, p) pair, a cell the (slot, bucket) id of the bucket-cell
// pass. Eight rounds fix the sort key of rank k1 = floor((n-1)*p) one byte
// at a time, most significant first: quantile_hist_kernel counts, per cell,
// the keys that share the prefix fixed so far into 256 bins of the next
// byte; quantile_pick_kernel walks the bins to the one holding the rank,
// appends its byte to the prefix and clears the bins. quantile_next_kernel
// then finds the rank's upper neighbour and quantile_finish_kernel decodes
// both. Every streaming pass reads cell (4 B) + value (8 B) per row and
// selection; the histogram is the only memory besides O(cells) state.
//
// Tile size and LDS span are a first choice, not a tuned one: 2048-row tiles
// (8 rows per thread, cell ids held in registers across selections) and a
// 16-cell x 256-bin u32 table = 16 KiB LDS, so four blocks per CU stay far
// inside the 160 KiB; the grid is capped at 1024 blocks = 256 CUs x 4.
// (series, ts)-sorted sources put a tile inside few cells; a tile that spans
// more than 16 cells (unsorted input) counts through global atomics instead;
// lds_cap (0..16) lowers that span at run time, 0 = global atomics only,
// which is how the two paths are timed against each other.
// Cell ids outside [0, n_cells) are skipped like -1.

// Loads the tile's cell ids into registers (-1 for rows past n or ids out of
// range) and reduces their span through s_lo/s_hi. Returns false when no row
// of the tile is kept. Every thread of the block must call it.
DEV_INLINE bool qsel_load_tile(const int32_t* __restrict__ cell, int64_t t0,
                               int64_t n, int n_cells, int32_t (&c)[QSEL_ROWS],
                               int32_t* s_lo, int32_t* s_hi,
                               int32_t& lo, int32_t& hi) {
  const int tid = threadIdx.x;
  if (tid == 0) { *s_lo = INT32_MAX; *s_hi = -1; }
  __syncthreads();
  int32_t my_lo = INT32_MAX, my_hi = -1;
#pragma unroll
  for (int j = 0; j < QSEL_ROWS; j++) {
    const int64_t i = t0 + (int64_t)j * QSEL_BLOCK + tid;
    int32_t v = -1;
    if (i < n) {
      v = cell[i];
      if (v < 0 || v >= n_cells) v = -1;
    }
    c[j] = v;
    if (v >= 0) { my_lo = min(my_lo, v); my_hi = max(my_hi, v); }
  }
  if (my_hi >= 0) {
    atomicMin(s_lo, my_lo);
    atomicMax(s_hi, my_hi);
  }
  __syncthreads();
  lo = *s_lo;
  hi = *s_hi;
  __syncthreads();
  return hi >= 0;
}

// hist: u32[Q, n_cells, 256]; prefix: u64[Q, n_cells]. pass 0..7, byte 0 is
// the most significant key byte.
__global__ void __launch_bounds__(QSEL_BLOCK) quantile_hist_kernel(
    const int32_t* __restrict__ cell,
    const double* __restrict__ fields, int64_t field_stride,
    const int32_t* __restrict__ field_idx, int n_field_rows,
    const int32_t* __restrict__ field_of_sel, int Q,
    int64_t n, int n_cells, int pass, int lds_cap,
    const unsigned long long* __restrict__ prefix,
    unsigned int* __restrict__ hist) {
  __shared__ int32_t s_lo, s_hi;
  __shared__ unsigned int s_hist[QSEL_LDS_CELLS * 256];
  __shared__ unsigned long long s_prefix[QSEL_LDS_CELLS];
  const int tid = threadIdx.x;
  const int hi_shift = 64 - 8 * pass;          // bits below the fixed prefix
  const int byte_shift = 56 - 8 * pass;
  const int64_t ntiles = (n + QSEL_TILE - 1) / QSEL_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t t0 = tile * QSEL_TILE;
    int32_t c[QSEL_ROWS];
    int32_t lo, hi;
    if (!qsel_load_tile(cell, t0, n, n_cells, c, &s_lo, &s_hi, lo, hi)) continue;
    const int range = hi - lo + 1;
    const bool in_lds = range <= lds_cap;
    for (int s = 0; s < Q; s++) {
      const int32_t frow = field_idx[field_of_sel[s]];
      if (frow < 0 || frow >= n_field_rows) continue;      // block-uniform
      const double* __restrict__ col = fields + (int64_t)frow * field_stride;
      const int64_t sbase = (int64_t)s * n_cells;
      if (in_lds) {
        for (int k = tid; k < range * 256; k += QSEL_BLOCK) s_hist[k] = 0u;
        if (tid < range) s_prefix[tid] = prefix[sbase + lo + tid];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < QSEL_ROWS; j++) {
          if (c[j] < 0) continue;
          const double v = col[t0 + (int64_t)j * QSEL_BLOCK + tid];
          if (isnan(v)) continue;
          const uint64_t key = f64_to_key(v);
          const int lc = c[j] - lo;
          if (pass > 0 && (key >> hi_shift) != (s_prefix[lc] >> hi_shift)) continue;
          atomicAdd(&s_hist[lc * 256 + (int)((key >> byte_shift) & 0xFF)], 1u);
        }
        __syncthreads();
        for (int k = tid; k < range * 256; k += QSEL_BLOCK) {
          const unsigned int h = s_hist[k];
          if (h) atomicAdd(&hist[(sbase + lo) * 256 + k], h);
        }
        __syncthreads();
      } else {
#pragma unroll
        for (int j = 0; j < QSEL_ROWS; j++) {
          if (c[j] < 0) continue;
          const double v = col[t0 + (int64_t)j * QSEL_BLOCK + tid];
          if (isnan(v)) continue;
          const uint64_t key = f64_to_key(v);
          const int64_t sc = sbase + c[j];
          if (pass > 0 && (key >> hi_shift) != (prefix[sc] >> hi_shift)) continue;
          atomicAdd(&hist[sc * 256 + (int)((key >> byte_shift) & 0xFF)], 1u);
        }
      }
    }
  }
}

// One wavefront per (selection, cell): lane l owns bins 4l..4l+3. Rows are
// fewer than 2^32 per call (checked by the binding), so u32 sums cannot wrap.
__global__ void __launch_bounds__(QSEL_BLOCK) quantile_pick_kernel(
    unsigned int* __restrict__ hist,           // [QC, 256], cleared on exit
    const double* __restrict__ p_of_sel, int n_cells, int64_t QC, int pass,
    unsigned long long* __restrict__ prefix,   // [QC]
    int64_t* __restrict__ k_left,              // [QC] rank still to find
    int64_t* __restrict__ k1_out,              // [QC] rank of pass 0
    int64_t* __restrict__ n_out) {             // [QC] non-NaN count
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * QSEL_BLOCK + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * QSEL_BLOCK) >> 6;
  for (int64_t idx = wave; idx < QC; idx += nwaves) {       // wave-uniform
    if (pass > 0 && n_out[idx] == 0) continue;
    uint4* bins4 = reinterpret_cast<uint4*>(hist + idx * 256) + lane;
    const uint4 b = *bins4;
    const unsigned int loc = b.x + b.y + b.z + b.w;
    unsigned int incl = loc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned int t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    const unsigned int total = __shfl(incl, 63, 64);
    int64_t k;
    if (pass == 0) {
      if (lane == 0) n_out[idx] = (int64_t)total;
      if (total == 0) continue;                // empty cell: left alone
      k = (int64_t)floor((double)((int64_t)total - 1) *
                         p_of_sel[(int)(idx / n_cells)]);
      if (lane == 0) k1_out[idx] = k;
    } else {
      k = k_left[idx];
    }
    const unsigned int excl = incl - loc;
    if ((int64_t)excl <= k && k < (int64_t)incl) {           // exactly one lane
      int64_t before = excl;
      int d = 4 * lane;
      if (k >= before + b.x) {
        before += b.x; d++;
        if (k >= before + b.y) {
          before += b.y; d++;
          if (k >= before + b.z) { before += b.z; d++; }
        }
      }
      prefix[idx] |= (unsigned long long)d << (56 - 8 * pass);
      k_left[idx] = k - before;
    }
    *bins4 = make_uint4(0u, 0u, 0u, 0u);
  }
}

// le[s, cell] += (key <= prefix); next[s, cell] = min key > prefix (init ~0).
__global__ void __launch_bounds__(QSEL_BLOCK) quantile_next_kernel(
    const int32_t* __restrict__ cell,
    const double* __restrict__ fields, int64_t field_stride,
    const int32_t* __restrict__ field_idx, int n_field_rows,
    const int32_t* __restrict__ field_of_sel, int Q,
    int64_t n, int n_cells, int lds_cap,
    const unsigned long long* __restrict__ prefix,
    unsigned long long* __restrict__ le,
    unsigned long long* __restrict__ next) {
  __shared__ int32_t s_lo, s_hi;
  __shared__ unsigned long long s_prefix[QSEL_LDS_CELLS];
  __shared__ unsigned long long s_next[QSEL_LDS_CELLS];
  __shared__ unsigned int s_le[QSEL_LDS_CELLS];
  const int tid = threadIdx.x;
  const int64_t ntiles = (n + QSEL_TILE - 1) / QSEL_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t t0 = tile * QSEL_TILE;
    int32_t c[QSEL_ROWS];
    int32_t lo, hi;
    if (!qsel_load_tile(cell, t0, n, n_cells, c, &s_lo, &s_hi, lo, hi)) continue;
    const int range = hi - lo + 1;
    const bool in_lds = range <= lds_cap;
    for (int s = 0; s < Q; s++) {
      const int32_t frow = field_idx[field_of_sel[s]];
      if (frow < 0 || frow >= n_field_rows) continue;      // block-uniform
      const double* __restrict__ col = fields + (int64_t)frow * field_stride;
      const int64_t sbase = (int64_t)s * n_cells;
      if (in_lds) {
        if (tid < range) {
          s_prefix[tid] = prefix[sbase + lo + tid];
          s_next[tid] = ~0ULL;
          s_le[tid] = 0u;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < QSEL_ROWS; j++) {
          if (c[j] < 0) continue;
          const double v = col[t0 + (int64_t)j * QSEL_BLOCK + tid];
          if (isnan(v)) continue;
          const uint64_t key = f64_to_key(v);
          const int lc = c[j] - lo;
          if (key <= s_prefix[lc]) atomicAdd(&s_le[lc], 1u);
          else atomicMin(&s_next[lc], (unsigned long long)key);
        }
        __syncthreads();
        if (tid < range) {
          if (s_le[tid]) atomicAdd(&le[sbase + lo + tid], (unsigned long long)s_le[tid]);
          if (s_next[tid] != ~0ULL) atomicMin(&next[sbase + lo + tid], s_next[tid]);
        }
        __syncthreads();
      } else {
#pragma unroll
        for (int j = 0; j < QSEL_ROWS; j++) {
          if (c[j] < 0) continue;
          const double v = col[t0 + (int64_t)j * QSEL_BLOCK + tid];
          if (isnan(v)) continue;
          const uint64_t key = f64_to_key(v);
          const int64_t sc = sbase + c[j];
          if (key <= prefix[sc]) atomicAdd(&le[sc], 1ULL);
          else atomicMin(&next[sc], (unsigned long long)key);
        }
      }
    }
  }
}

// lo = value of rank k1, hi = value of rank min(k1+1, n-1); NaN where n == 0.
__global__ void quantile_finish_kernel(
    const unsigned long long* __restrict__ prefix,
    const int64_t* __restrict__ k1, const int64_t* __restrict__ cnt,
    const unsigned long long* __restrict__ le,
    const unsigned long long* __restrict__ next,
    int64_t QC, double* __restrict__ out_lo, double* __restrict__ out_hi) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < QC; i += stride) {
    if (cnt[i] == 0) {
      out_lo[i] = quiet_nan();
      out_hi[i] = quiet_nan();
      continue;
    }
    const double lo = key_to_f64(prefix[i]);
    const bool same = (k1[i] + 1 < (int64_t)le[i]) || next[i] == ~0ULL;
    out_lo[i] = lo;
    out_hi[i] = same ? lo : key_to_f64(next[i]);
  }
}

// ------------------------------------------- K22 grouped two-pass moments
//
// Second moments per (selection, cell): a selection is a pair of field
// columns (x, y), x == y being the one-argument form; a row counts where its
// cell is valid and neither value is NaN (pairwise deletion). Two streaming
// passes in the shape of field_bucket_agg_lds_kernel (AGG_TILE-row tiles,
// coalesced loads, the tile's cell span privatised in LDS, global atomics
// when the span exceeds lds_cap), one selection at a time:
//   moments_sums_kernel    : pair count, sum x, sum y, min/max keys of x, y
//   moments_mean_kernel    : means and the exact constant flags, per cell
//   moments_centred_kernel : sum (x-mx)^2, sum (y-my)^2, sum (x-mx)(y-my)
// Summing squares of raw values would cancel catastrophically for data far
// from zero; centring on the mean of pass 1 keeps every term small.
// LDS: pass 1 holds a u32 count and six 8-byte tables (52 KiB, three blocks
// per CU inside 160 KiB), pass 2 a u32 count and three f64 tables (28 KiB).
// A selection with x == y reads one column and fills only the x planes; the
// binding copies them to the y planes.
// Cell ids outside [0, n_cells) are skipped like -1.

// The tile's span of valid cell ids through s_lo/s_hi; false when no row of
// the tile is kept. Every thread of the block must call it.
DEV_INLINE bool moments_tile_span(const int32_t* __restrict__ cell, int64_t t0,
                                  int64_t t1, int n_cells, int32_t* s_lo,
                                  int32_t* s_hi, int32_t& lo, int32_t& hi) {
  const int tid = threadIdx.x;
  if (tid == 0) { *s_lo = INT32_MAX; *s_hi = -1; }
  __syncthreads();
  int32_t my_lo = INT32_MAX, my_hi = -1;
  for (int64_t i = t0 + tid; i < t1; i += blockDim.x) {
    const int32_t c = cell[i];
    if (c >= 0 && c < n_cells) { my_lo = min(my_lo, c); my_hi = max(my_hi, c); }
  }
  if (my_hi >= 0) {
    atomicMin(s_lo, my_lo);
    atomicMax(s_hi, my_hi);
  }
  __syncthreads();
  lo = *s_lo;
  hi = *s_hi;
  __syncthreads();
  return hi >= 0;
}

// Order key of a value for the constant test: -0.0 and 0.0 compare equal as
// numbers, so both take the key of 0.0.
DEV_INLINE unsigned long long moments_key(double v) {
  return (unsigned long long)f64_to_key(v == 0.0 ? 0.0 : v);
}

// Planes are [M, n_cells]; min keys start at u64 max, everything else at 0.
__global__ void __launch_bounds__(256) moments_sums_kernel(
    const int32_t* __restrict__ cell,
    const double* __restrict__ fields, int64_t field_stride,
    const int32_t* __restrict__ field_idx, int n_field_rows,
    const int32_t* __restrict__ fx_of_sel, const int32_t* __restrict__ fy_of_sel,
    int M, int64_t n, int n_cells, int lds_cap,
    unsigned long long* __restrict__ out_n,
    double* __restrict__ out_sx, double* __restrict__ out_sy,
    unsigned long long* __restrict__ out_minx,
    unsigned long long* __restrict__ out_maxx,
    unsigned long long* __restrict__ out_miny,
    unsigned long long* __restrict__ out_maxy) {
  __shared__ int32_t s_lo, s_hi;
  __shared__ unsigned int s_cnt[LDS_CELLS];
  __shared__ double s_sx[LDS_CELLS];
  __shared__ double s_sy[LDS_CELLS];
  __shared__ unsigned long long s_minx[LDS_CELLS];
  __shared__ unsigned long long s_maxx[LDS_CELLS];
  __shared__ unsigned long long s_miny[LDS_CELLS];
  __shared__ unsigned long long s_maxy[LDS_CELLS];
  const int tid = threadIdx.x;
  const int nthreads = blockDim.x;
  const int64_t ntiles = (n + AGG_TILE - 1) / AGG_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t t0 = tile * AGG_TILE;
    const int64_t t1 = min(t0 + (int64_t)AGG_TILE, n);
    int32_t lo, hi;
    if (!moments_tile_span(cell, t0, t1, n_cells, &s_lo, &s_hi, lo, hi)) continue;
    const int range = hi - lo + 1;
    const bool in_lds = range <= lds_cap;
    for (int s = 0; s < M; s++) {
      const int32_t rx = field_idx[fx_of_sel[s]];
      const int32_t ry = field_idx[fy_of_sel[s]];
      if (rx < 0 || rx >= n_field_rows || ry < 0 || ry >= n_field_rows)
        continue;                                          // block-uniform
      const bool same = fx_of_sel[s] == fy_of_sel[s];
      const double* __restrict__ colx = fields + (int64_t)rx * field_stride;
      const double* __restrict__ coly = fields + (int64_t)ry * field_stride;
      const int64_t sbase = (int64_t)s * n_cells;
      if (in_lds) {
        for (int k = tid; k < range; k += nthreads) {
          s_cnt[k] = 0u; s_sx[k] = 0.0; s_sy[k] = 0.0;
          s_minx[k] = ~0ULL; s_maxx[k] = 0ULL;
          s_miny[k] = ~0ULL; s_maxy[k] = 0ULL;
        }
        __syncthreads();
        for (int64_t i = t0 + tid; i < t1; i += nthreads) {
          const int32_t c = cell[i];
          if (c < 0 || c >= n_cells) continue;
          const double x = colx[i];
          const double y = same ? x : coly[i];
          if (isnan(x) || isnan(y)) continue;
          const int k = c - lo;
          atomicAdd(&s_cnt[k], 1u);
          atomicAdd(&s_sx[k], x);
          const unsigned long long kx = moments_key(x);
          atomicMin(&s_minx[k], kx);
          atomicMax(&s_maxx[k], kx);
          if (!same) {
            atomicAdd(&s_sy[k], y);
            const unsigned long long ky = moments_key(y);
            atomicMin(&s_miny[k], ky);
            atomicMax(&s_maxy[k], ky);
          }
        }
        __syncthreads();
        for (int k = tid; k < range; k += nthreads) {
          if (!s_cnt[k]) continue;
          const int64_t o = sbase + lo + k;
          atomicAdd(&out_n[o], (unsigned long long)s_cnt[k]);
          atomicAdd(&out_sx[o], s_sx[k]);
          atomicMin(&out_minx[o], s_minx[k]);
          atomicMax(&out_maxx[o], s_maxx[k]);
          if (!same) {
            atomicAdd(&out_sy[o], s_sy[k]);
            atomicMin(&out_miny[o], s_miny[k]);
            atomicMax(&out_maxy[o], s_maxy[k]);
          }
        }
        __syncthreads();
      } else {
        for (int64_t i = t0 + tid; i < t1; i += nthreads) {
          const int32_t c = cell[i];
          if (c < 0 || c >= n_cells) continue;
          const double x = colx[i];
          const double y = same ? x : coly[i];
          if (isnan(x) || isnan(y)) continue;
          const int64_t o = sbase + c;
          atomicAdd(&out_n[o], 1ULL);
          atomicAdd(&out_sx[o], x);
          const unsigned long long kx = moments_key(x);
          atomicMin(&out_minx[o], kx);
          atomicMax(&out_maxx[o], kx);
          if (!same) {
            atomicAdd(&out_sy[o], y);
            const unsigned long long ky = moments_key(y);
            atomicMin(&out_miny[o], ky);
            atomicMax(&out_maxy[o], ky);
          }
        }
      }
    }
  }
}

// Means and constant flags of every (selection, cell), after the last source
// of pass 1. A constant column's mean is the value itself, not sum / n, so
// that pass 2 sees x - mean == 0 exactly. n == 0: NaN means, flags clear.
__global__ void moments_mean_kernel(
    const unsigned long long* __restrict__ cnt,
    const double* __restrict__ sx, const double* __restrict__ sy,
    const unsigned long long* __restrict__ minx,
    const unsigned long long* __restrict__ maxx,
    const unsigned long long* __restrict__ miny,
    const unsigned long long* __restrict__ maxy,
    const int32_t* __restrict__ fx_of_sel, const int32_t* __restrict__ fy_of_sel,
    int n_cells, int64_t MC,
    double* __restrict__ mean_x, double* __restrict__ mean_y,
    bool* __restrict__ const_x, bool* __restrict__ const_y) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < MC; i += stride) {
    const unsigned long long c = cnt[i];
    if (c == 0) {
      mean_x[i] = quiet_nan(); mean_y[i] = quiet_nan();
      const_x[i] = false; const_y[i] = false;
      continue;
    }
    const int s = (int)(i / n_cells);
    const bool cx = minx[i] == maxx[i];
    const double mx = cx ? key_to_f64(minx[i]) : sx[i] / (double)c;
    mean_x[i] = mx;
    const_x[i] = cx;
    if (fx_of_sel[s] == fy_of_sel[s]) {
      mean_y[i] = mx;
      const_y[i] = cx;
    } else {
      const bool cy = miny[i] == maxy[i];
      mean_y[i] = cy ? key_to_f64(miny[i]) : sy[i] / (double)c;
      const_y[i] = cy;
    }
  }
}

__global__ void __launch_bounds__(256) moments_centred_kernel(
    const int32_t* __restrict__ cell,
    const double* __restrict__ fields, int64_t field_stride,
    const int32_t* __restrict__ field_idx, int n_field_rows,
    const int32_t* __restrict__ fx_of_sel, const int32_t* __restrict__ fy_of_sel,
    int M, int64_t n, int n_cells, int lds_cap,
    const double* __restrict__ mean_x, const double* __restrict__ mean_y,
    double* __restrict__ out_m2x, double* __restrict__ out_m2y,
    double* __restrict__ out_cxy) {
  __shared__ int32_t s_lo, s_hi;
  __shared__ unsigned int s_cnt[LDS_CELLS];
  __shared__ double s_m2x[LDS_CELLS];
  __shared__ double s_m2y[LDS_CELLS];
  __shared__ double s_cxy[LDS_CELLS];
  const int tid = threadIdx.x;
  const int nthreads = blockDim.x;
  const int64_t ntiles = (n + AGG_TILE - 1) / AGG_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t t0 = tile * AGG_TILE;
    const int64_t t1 = min(t0 + (int64_t)AGG_TILE, n);
    int32_t lo, hi;
    if (!moments_tile_span(cell, t0, t1, n_cells, &s_lo, &s_hi, lo, hi)) continue;
    const int range = hi - lo + 1;
    const bool in_lds = range <= lds_cap;
    for (int s = 0; s < M; s++) {
      const int32_t rx = field_idx[fx_of_sel[s]];
      const int32_t ry = field_idx[fy_of_sel[s]];
      if (rx < 0 || rx >= n_field_rows || ry < 0 || ry >= n_field_rows)
        continue;                                          // block-uniform
      const bool same = fx_of_sel[s] == fy_of_sel[s];
      const double* __restrict__ colx = fields + (int64_t)rx * field_stride;
      const double* __restrict__ coly = fields + (int64_t)ry * field_stride;
      const int64_t sbase = (int64_t)s * n_cells;
      if (in_lds) {
        for (int k = tid; k < range; k += nthreads) {
          s_cnt[k] = 0u; s_m2x[k] = 0.0; s_m2y[k] = 0.0; s_cxy[k] = 0.0;
        }
        __syncthreads();
        for (int64_t i = t0 + tid; i < t1; i += nthreads) {
          const int32_t c = cell[i];
          if (c < 0 || c >= n_cells) continue;
          const double x = colx[i];
          const double y = same ? x : coly[i];
          if (isnan(x) || isnan(y)) continue;
          const int k = c - lo;
          const double dx = x - mean_x[sbase + c];
          atomicAdd(&s_cnt[k], 1u);
          atomicAdd(&s_m2x[k], dx * dx);
          if (!same) {
            const double dy = y - mean_y[sbase + c];
            atomicAdd(&s_m2y[k], dy * dy);
            atomicAdd(&s_cxy[k], dx * dy);
          }
        }
        __syncthreads();
        for (int k = tid; k < range; k += nthreads) {
          if (!s_cnt[k]) continue;
          const int64_t o = sbase + lo + k;
          atomicAdd(&out_m2x[o], s_m2x[k]);
          if (!same) {
            atomicAdd(&out_m2y[o], s_m2y[k]);
            atomicAdd(&out_cxy[o], s_cxy[k]);
          }
        }
        __syncthreads();
      } else {
        for (int64_t i = t0 + tid; i < t1; i += nthreads) {
          const int32_t c = cell[i];
          if (c < 0 || c >= n_cells) continue;
          const double x = colx[i];
          const double y = same ? x : coly[i];
          if (isnan(x) || isnan(y)) continue;
          const int64_t o = sbase + c;
          const double dx = x - mean_x[o];
          atomicAdd(&out_m2x[o], dx * dx);
          if (!same) {
            const double dy = y - mean_y[o];
            atomicAdd(&out_m2y[o], dy * dy);
            atomicAdd(&out_cxy[o], dx * dy);
          }
        }
      }
    }
  }
}

// ------------------------------------------------- K16 scatter append
/// One launch appends a routed wire batch into MULTIPLE region memtables:
// row i goes to region region_of[i] at row dst_off[i]. Replaces per-region
// narrow+copy_ chains (two dozen small torch dispatches per batch) with a
// single kernel — the ingest hot path's device side.
__global__ void scatter_append_kernel(
    const int64_t* __restrict__ ts,
    const int32_t* __restrict__ series,
    const double* __restrict__ fields,        // [nf, n] row-major
    const int32_t* __restrict__ region_of,
    const int64_t* __restrict__ dst_off,
    int64_t* const* __restrict__ ts_ptrs,     // [R]
    int32_t* const* __restrict__ se_ptrs,
    double* const* __restrict__ f_ptrs,
    const int64_t* __restrict__ strides,      // [R] field stride (cap)
    int nf, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int r = region_of[i];
    const int64_t o = dst_off[i];
    ts_ptrs[r][o] = ts[i];
    se_ptrs[r][o] = series[i];
    double* __restrict__ fp = f_ptrs[r];
    const int64_t st = strides[r];
    for (int f = 0; f < nf; f++) {
      fp[(int64_t)f * st + o] = fields[(int64_t)f * n + i];
    }
  }
}

// Packed form of K16: the whole routed batch arrives as ONE block (layout of
// gdb_ingest::StageLayout in csrc/ingest_core.h, every segment 8-byte
// aligned):
//   ts i64[n] | fields f64[nf*n] | dst_off i64[n] | series i32[n] | region i32[n]
// and the per-region destinations travel by value in the kernel arguments,
// so a batch costs one H2D copy and one launch with no pointer-table upload.
// Row i lands at base[region[i]] + dst_off[i]. Work items run over
// (column, row) with row fastest: column 0 writes ts + series, column 1 + f
// writes field f — reads stay coalesced along the row axis and rows of one
// region write neighbouring addresses.
__global__ void scatter_append_packed_kernel(
    const unsigned char* __restrict__ stage, int64_t n, int nf,
    const PackedRegions regs) {
  const int64_t* __restrict__ ts = reinterpret_cast<const int64_t*>(stage);
  const double* __restrict__ fields = reinterpret_cast<const double*>(stage + 8 * n);
  const int64_t* __restrict__ dst_off =
      reinterpret_cast<const int64_t*>(stage + 8 * n + 8 * (int64_t)nf * n);
  const int64_t i32_bytes = (4 * n + 7) & ~(int64_t)7;
  const unsigned char* sbase = stage + 16 * n + 8 * (int64_t)nf * n;
  const int32_t* __restrict__ series = reinterpret_cast<const int32_t*>(sbase);
  const int32_t* __restrict__ region = reinterpret_cast<const int32_t*>(sbase + i32_bytes);
  const int64_t total = n * (int64_t)(nf + 1);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += stride) {
    const int64_t col = idx / n;
    const int64_t i = idx - col * n;
    const int r = region[i];
    const int64_t o = regs.base[r] + dst_off[i];
    if (col == 0) {
      regs.ts[r][o] = ts[i];
      regs.se[r][o] = series[i];
    } else {
      const int64_t f = col - 1;
      regs.f[r][f * regs.stride[r] + o] = fields[f * n + i];
    }
  }
}

// ------------------------------------------------- K11 RLE/bit-packed expand
// Parquet hybrid RLE/bit-packed dictionary indices → i32, fully parallel:
// one thread per OUTPUT element; the run covering the element is found by
// binary search over the host-built run table (csrc/pagedec.cpp), then
// either the RLE constant is written or `bw` bits are extracted at the
// element's bit offset. Branchy page parsing stays on the host; the
// bandwidth-bound expansion runs at HBM speed here.
__global__ void rle_expand_indices_kernel(
    const int64_t* __restrict__ runs,   // [R,5] is_packed, off, val, out_start, count
    int64_t R,
    const uint8_t* __restrict__ blob,
    int bw,
    int32_t* __restrict__ out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    // binary search: last run with out_start <= i
    int64_t lo = 0, hi = R - 1;
    while (lo < hi) {
      int64_t mid = (lo + hi + 1) >> 1;
      if (runs[mid * 5 + 3] <= i) lo = mid; else hi = mid - 1;
    }
    const int64_t* run = runs + lo * 5;
    if (run[0] == 0) {
      out[i] = (int32_t)run[2];
    } else {
      const int64_t rel = i - run[3];
      const int64_t bit = rel * bw;
      const uint8_t* p = blob + run[1] + (bit >> 3);
      // assemble up to 40 bits (bw <= 32) from unaligned bytes
      uint64_t v = (uint64_t)p[0] | ((uint64_t)p[1] << 8) |
                   ((uint64_t)p[2] << 16) | ((uint64_t)p[3] << 24) |
                   ((uint64_t)p[4] << 32);
      out[i] = (int32_t)((v >> (bit & 7)) & ((bw >= 32) ? 0xFFFFFFFFULL
                                                        : ((1ULL << bw) - 1)));
    }
  }
}

// ------------------------------------------------------ K20 Gorilla / delta
// Block format (engine/gorilla.py is the specification; its pack() is the
// host packer and the encoder kernels below write the same bytes). Widths
// are fixed per block, so every value's bit position is O(1) and both
// directions run one thread per value / per output word.
// Layout per block of `count` values in `blob` (blocks start 8B-aligned):
//   [i64 base_ts][u64 base_val][u8 ts_bits][u8 val_bits][u16 count]
//   [u8 val_mode][u8 scale_k][2B pad]                          (24 bytes)
//   [count-1 × zigzag(ts[i] - base_ts), ts_bits each, LSB first, pad to 8B]
//   [count-1 × value payload, val_bits each, LSB first, pad to 8B]
// val_mode 0: base_val = bits(val[0]), payload = bits(val[i]) ^ base_val.
// val_mode 1: base_val = (i64)rint(val[0]·10^scale_k), payload =
//   zigzag(rint(val[i]·10^scale_k) - base_val); decodes as int / 10^scale_k.
// Deltas are ABSOLUTE from the block base (not delta-of-delta), so no
// prefix sum is needed. The blob ends in 16 zero bytes: the decoder reads
// up to 9 bytes past the last packed bit.
__global__ void gorilla_decode_kernel(
    const uint8_t* __restrict__ blob,
    const int64_t* __restrict__ block_off,   // [B] byte offset of each block
    const int64_t* __restrict__ out_off,     // [B] first output index
    int64_t B,
    int64_t* __restrict__ out_ts,
    double* __restrict__ out_val,
    int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t total_threads = stride;
  (void)total_threads;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;; g += stride) {
    // map thread → (block, element) via flat index over n
    if (g >= n) return;
    // find block by binary search on out_off
    int64_t lo = 0, hi = B - 1;
    while (lo < hi) {
      int64_t mid = (lo + hi + 1) >> 1;
      if (out_off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const uint8_t* blk = blob + block_off[lo];
    int64_t base_ts;
    uint64_t base_val;
    memcpy(&base_ts, blk, 8);
    memcpy(&base_val, blk + 8, 8);
    const int ts_bits = blk[16];
    const int val_bits = blk[17];
    uint16_t count;
    memcpy(&count, blk + 18, 2);
    const int val_mode = blk[20];   // 0 = XOR f64, 1 = scaled int delta
    const int scale_k = blk[21];
    double scale = 1.0;                 // 10^k exact in f64 for k <= 4
    for (int q = 0; q < scale_k; q++) scale *= 10.0;
    const uint8_t* ts_data = blk + 24;
    const int64_t rel = g - out_off[lo];
    if (rel >= count) continue;
    if (rel == 0) {
      out_ts[g] = base_ts;
      out_val[g] = (val_mode == 1)
          ? (double)(int64_t)base_val / scale
          : __longlong_as_double((long long)base_val);
      continue;
    }
    const int64_t k = rel - 1;   // packed arrays hold values 1..count-1
    // absolute zigzagged delta from base, ts_bits each
    uint64_t tsv = 0;
    if (ts_bits) {
      const int64_t bit = k * ts_bits;
      const uint8_t* p = ts_data + (bit >> 3);
      const int sft = (int)(bit & 7);
      uint64_t w0 = 0;
      for (int b = 0; b < 8; b++) w0 |= (uint64_t)p[b] << (8 * b);
      uint64_t v = w0 >> sft;
      if (sft) v |= (uint64_t)p[8] << (64 - sft);   // spillover bits 64..70
      tsv = v & ((ts_bits >= 64) ? ~0ULL : ((1ULL << ts_bits) - 1));
    }
    const int64_t dz = (int64_t)(tsv >> 1) ^ -(int64_t)(tsv & 1);
    out_ts[g] = base_ts + dz;
    const int64_t ts_bytes = ((int64_t)(count - 1) * ts_bits + 7) / 8;
    const uint8_t* val_data = ts_data + ((ts_bytes + 7) / 8) * 8;
    uint64_t xv = 0;
    if (val_bits) {
      const int64_t bit = k * val_bits;
      const uint8_t* p = val_data + (bit >> 3);
      const int sft = (int)(bit & 7);
      uint64_t w0 = 0;
      for (int b = 0; b < 8; b++) w0 |= (uint64_t)p[b] << (8 * b);
      uint64_t v = w0 >> sft;
      if (sft) v |= (uint64_t)p[8] << (64 - sft);
      xv = v & ((val_bits >= 64) ? ~0ULL : ((1ULL << val_bits) - 1));
    }
    if (val_mode == 1) {
      const int64_t dvz = (int64_t)(xv >> 1) ^ -(int64_t)(xv & 1);
      out_val[g] = (double)((int64_t)base_val + dvz) / scale;
    } else {
      out_val[g] = __longlong_as_double((long long)(base_val ^ xv));
    }
  }
}

// ------------------------------------------------------------ K20 encoder
// Three launches write what gorilla.pack() writes, byte for byte:
//   gorilla_scale_kernel  : one reduction over the column → which 10^k
//                           scales (k = 0..4) reproduce every value;
//   gorilla_widths_kernel : one workgroup per codec block → ts_bits,
//                           val_bits and the block's byte size;
//   gorilla_write_kernel  : one workgroup per codec block → header, then
//                           each thread gathers the values overlapping its
//                           64-bit output word from LDS and stores it whole.
// The exclusive scan of the sizes between the last two runs in the binding.
constexpr int GENC_THREADS = 256;
constexpr unsigned GENC_NONFINITE = 1u << 5;
constexpr unsigned GENC_ALL_SCALES = 0x1Fu;

DEV_INLINE uint64_t zigzag64(int64_t d) {
  return ((uint64_t)d << 1) ^ (uint64_t)(d >> 63);
}

DEV_INLINE double gorilla_pow10(int k) {   // exact in f64 for k <= 4
  double s = 1.0;
  for (int q = 0; q < k; q++) s *= 10.0;
  return s;
}

// fail word → (val_mode, scale_k). No value column packs like a column of
// zeros: scaled mode at k = 0.
DEV_INLINE void gorilla_mode(const double* vals, const unsigned* fail,
                             int& val_mode, int& scale_k) {
  val_mode = 1;
  scale_k = 0;
  if (vals == nullptr) return;
  const unsigned f = *fail;
  if (!(f & GENC_NONFINITE)) {
    for (int k = 0; k < 5; k++) {
      if (!((f >> k) & 1u)) { scale_k = k; return; }
    }
  }
  val_mode = 0;
}

// gorilla._detect_scale: bit k of *fail is set when some value does not
// survive (double)(int64)rint(v·10^k) / 10^k bit for bit, or |v·10^k| is
// not below 2^47; GENC_NONFINITE when some value is NaN or ±inf. The
// multiply, rint and divide are separately rounded IEEE operations.
__global__ void __launch_bounds__(GENC_THREADS) gorilla_scale_kernel(
    const double* __restrict__ vals, int64_t n, unsigned* __restrict__ fail) {
#pragma clang fp contract(off)
  unsigned f = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const double v = vals[i];
    const uint64_t bits = (uint64_t)__double_as_longlong(v);
    if ((bits & 0x7FF0000000000000ULL) == 0x7FF0000000000000ULL) {
      f |= GENC_NONFINITE | GENC_ALL_SCALES;
      continue;
    }
    double scale = 1.0;
    for (int k = 0; k < 5; k++) {
      const double sv = v * scale;
      // an out-of-range (or overflowed) product is never converted
      if (!(fabs(sv) < 140737488355328.0)) {          // 2^47
        f |= 1u << k;
      } else {
        const double back = (double)(int64_t)rint(sv) / scale;
        if ((uint64_t)__double_as_longlong(back) != bits) f |= 1u << k;
      }
      scale *= 10.0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) f |= __shfl_xor(f, off, 64);
  if ((threadIdx.x & 63) == 0 && f) atomicOr(fail, f);
}

// payload of value i of the codec block starting at row s
DEV_INLINE uint64_t gorilla_val_payload(const double* __restrict__ vals,
                                        int64_t s, int64_t i, int val_mode,
                                        double scale) {
#pragma clang fp contract(off)
  if (vals == nullptr) return 0;
  if (val_mode == 1) {
    // scaled mode was chosen, so every product is finite and below 2^47
    const int64_t base = (int64_t)rint(vals[s] * scale);
    return zigzag64((int64_t)rint(vals[i] * scale) - base);
  }
  return (uint64_t)__double_as_longlong(vals[i]) ^
         (uint64_t)__double_as_longlong(vals[s]);
}

DEV_INLINE uint64_t gorilla_ts_payload(const int64_t* __restrict__ ts,
                                       int64_t s, int64_t i) {
  // wrap-around difference, like numpy's int64
  return zigzag64((int64_t)((uint64_t)ts[i] - (uint64_t)ts[s]));
}

DEV_INLINE int bit_length64(uint64_t x) { return x ? 64 - __clzll(x) : 0; }

// bits[2b] = ts_bits, bits[2b+1] = val_bits, sizes[b] = bytes of block b.
// bit_length(max) == bit_length(OR), so the widths are an OR reduction.
__global__ void __launch_bounds__(GENC_THREADS) gorilla_widths_kernel(
    const int64_t* __restrict__ ts, const double* __restrict__ vals,
    int64_t n, int block, int pack_ts, const unsigned* __restrict__ fail,
    uint8_t* __restrict__ bits, int64_t* __restrict__ sizes) {
  __shared__ uint64_t red[2][GENC_THREADS / 64];
  const int64_t s = (int64_t)blockIdx.x * block;
  const int count = (int)((n - s < block) ? (n - s) : block);
  int val_mode, scale_k;
  gorilla_mode(vals, fail, val_mode, scale_k);
  const double scale = gorilla_pow10(scale_k);
  uint64_t or_ts = 0, or_val = 0;
  for (int r = 1 + (int)threadIdx.x; r < count; r += GENC_THREADS) {
    if (pack_ts) or_ts |= gorilla_ts_payload(ts, s, s + r);
    or_val |= gorilla_val_payload(vals, s, s + r, val_mode, scale);
  }
  for (int off = 32; off > 0; off >>= 1) {
    or_ts |= __shfl_xor(or_ts, off, 64);
    or_val |= __shfl_xor(or_val, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = or_ts;
    red[1][threadIdx.x >> 6] = or_val;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < GENC_THREADS / 64; w++) {
      or_ts |= red[0][w];
      or_val |= red[1][w];
    }
    const int tb = bit_length64(or_ts), vb = bit_length64(or_val);
    const int64_t k = count - 1;
    bits[2 * (int64_t)blockIdx.x] = (uint8_t)tb;
    bits[2 * (int64_t)blockIdx.x + 1] = (uint8_t)vb;
    sizes[blockIdx.x] = 24 + 8 * ((k * tb + 63) / 64) + 8 * ((k * vb + 63) / 64);
  }
}

// k values of w bits each (staged in LDS, no bits above w) → ceil(k·w/64)
// whole little-endian words; bits past the last value are zero.
DEV_INLINE void gorilla_pack_section(const uint64_t* stage, int k, int w,
                                     uint64_t* __restrict__ out) {
  const int words = (k * w + 63) >> 6;
  for (int j = (int)threadIdx.x; j < words; j += GENC_THREADS) {
    const int lo = j << 6;
    uint64_t acc = 0;
    for (int i = lo / w; i < k && i * w < lo + 64; i++) {
      const int sh = i * w - lo;             // -63 .. 63
      const uint64_t v = stage[i];
      acc |= (sh >= 0) ? (v << sh) : (v >> -sh);
    }
    out[j] = acc;
  }
}

__global__ void __launch_bounds__(GENC_THREADS) gorilla_write_kernel(
    const int64_t* __restrict__ ts, const double* __restrict__ vals,
    int64_t n, int block, const unsigned* __restrict__ fail,
    const uint8_t* __restrict__ bits, const int64_t* __restrict__ block_off,
    uint8_t* __restrict__ blob) {
  __shared__ uint64_t stage[GENC_MAX_BLOCK];
  const int64_t s = (int64_t)blockIdx.x * block;
  const int count = (int)((n - s < block) ? (n - s) : block);
  const int k = count - 1;
  int val_mode, scale_k;
  gorilla_mode(vals, fail, val_mode, scale_k);
  const double scale = gorilla_pow10(scale_k);
  const int tb = bits[2 * (int64_t)blockIdx.x];
  const int vb = bits[2 * (int64_t)blockIdx.x + 1];
  // block offsets are sums of multiples of 8, so every store is aligned
  uint64_t* out = reinterpret_cast<uint64_t*>(blob + block_off[blockIdx.x]);
  if (threadIdx.x == 0) {
    uint64_t base_val = 0;
    if (vals != nullptr) {
#pragma clang fp contract(off)
      base_val = (val_mode == 1)
          ? (uint64_t)(int64_t)rint(vals[s] * scale)
          : (uint64_t)__double_as_longlong(vals[s]);
    }
    out[0] = (uint64_t)ts[s];
    out[1] = base_val;
    out[2] = (uint64_t)tb | ((uint64_t)vb << 8) | ((uint64_t)count << 16) |
             ((uint64_t)val_mode << 32) | ((uint64_t)scale_k << 40);
  }
  out += 3;
  if (tb) {                                   // uniform across the workgroup
    for (int r = (int)threadIdx.x; r < k; r += GENC_THREADS)
      stage[r] = gorilla_ts_payload(ts, s, s + 1 + r);
    __syncthreads();
    gorilla_pack_section(stage, k, tb, out);
    __syncthreads();
    out += (k * tb + 63) >> 6;
  }
  if (vb) {
    for (int r = (int)threadIdx.x; r < k; r += GENC_THREADS)
      stage[r] = gorilla_val_payload(vals, s, s + 1 + r, val_mode, scale);
    __syncthreads();
    gorilla_pack_section(stage, k, vb, out);
  }
}

// ---------------------------------------------------------------- launchers
// Defined by qualified name: a definition that matches no declaration of
// kernels.h is a compile error, not a new overload.

static inline int grid_for(int64_t n, int block) {
  int64_t g = (n + block - 1) / block;
  if (g > 2048) g = 2048;  // G11: cap + grid-stride
  if (g < 1) g = 1;
  return (int)g;
}

static inline int qsel_grid(int64_t n) {
  const int64_t ntiles = (n + QSEL_TILE - 1) / QSEL_TILE;
  return (int)max(min(ntiles, (int64_t)QSEL_MAX_GRID), (int64_t)1);
}

// one block per AGG_TILE rows, like the bucket aggregate
static inline int moments_grid(int64_t n) {
  const int64_t ntiles = (n + AGG_TILE - 1) / AGG_TILE;
  return (int)max(min(ntiles, (int64_t)8192), (int64_t)1);
}

}  // namespace gdb_hip

void gdb_hip::launch_decode_minmax(
    const unsigned long long* minkey, const unsigned long long* maxkey,
    const unsigned long long* cnt, double* out_min, double* out_max,
    int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(decode_minmax_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream,
      minkey, maxkey, cnt, out_min, out_max, n);
}

void gdb_hip::launch_filter_series_time(
    const int64_t* ts, const int32_t* series, const int32_t* slot_lut,
    int lut_size, int64_t ts_lo, int64_t ts_hi, int64_t n, bool* keep,
    hipStream_t stream) {
  hipLaunchKernelGGL(filter_series_time_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream,
      ts, series, slot_lut, lut_size, ts_lo, ts_hi, n, keep);
}

void gdb_hip::launch_dedup_mark_last(
    const int32_t* series, const int64_t* ts, int64_t n, bool* keep,
    hipStream_t stream) {
  hipLaunchKernelGGL(dedup_mark_last_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream,
      series, ts, n, keep);
}

void gdb_hip::launch_merge_last_non_null(
    const int64_t* kidx, int64_t g, const double* fields, int64_t field_stride,
    int nf, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(merge_last_non_null_kernel, dim3(grid_for(g, 256)), dim3(256), 0, stream,
      kidx, g, fields, field_stride, nf, out);
}

void gdb_hip::launch_ts_bucket_agg(
    const int64_t* ts, const int32_t* series, const double* fields,
    int64_t field_stride, const int32_t* field_idx, int nf,
    const int32_t* slot_lut, int lut_size,
    int64_t ts_lo, int64_t ts_hi, int64_t origin, int64_t bucket_ms,
    int n_slots, int n_buckets, int64_t n,
    int32_t* cell_buf,
    double* out_sum, unsigned long long* out_cnt,
    unsigned long long* out_min, unsigned long long* out_max,
    unsigned long long* out_rows, hipStream_t stream) {
  launch_bucket_cells(ts, series, slot_lut, lut_size, ts_lo, ts_hi, origin,
                      bucket_ms, n_buckets, n, cell_buf, stream);
  // Tiles beyond the grid are taken by the kernel's tile grid-stride loop
  // (only past 8192 tiles = 67M rows, too large for the test suite).
  // n == 0 would give a zero-sized grid, which HIP rejects: clamp to 1.
  const int64_t ntiles = (n + AGG_TILE - 1) / AGG_TILE;
  const int grid = (int)max(min(ntiles, (int64_t)8192), (int64_t)1);
  hipLaunchKernelGGL(field_bucket_agg_lds_kernel,
      dim3(grid), dim3(256), 0, stream,
      cell_buf, fields, field_stride, field_idx, nf, n,
      (int64_t)n_slots * n_buckets,
      out_sum, out_cnt, out_min, out_max, out_rows);
}

void gdb_hip::launch_scatter_append(
    const int64_t* ts, const int32_t* series, const double* fields,
    const int32_t* region_of, const int64_t* dst_off,
    int64_t* const* ts_ptrs, int32_t* const* se_ptrs, double* const* f_ptrs,
    const int64_t* strides, int nf, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(scatter_append_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream,
      ts, series, fields, region_of, dst_off, ts_ptrs, se_ptrs, f_ptrs,
      strides, nf, n);
}

void gdb_hip::launch_scatter_append_packed(
    const unsigned char* stage, int64_t n, int nf, const PackedRegions& regs,
    hipStream_t stream) {
  hipLaunchKernelGGL(scatter_append_packed_kernel,
      dim3(grid_for(n * (int64_t)(nf + 1), 256)), dim3(256), 0, stream,
      stage, n, nf, regs);
}

void gdb_hip::launch_series_last(
    const int64_t* ts, const int32_t* series, const int32_t* slot_lut,
    int lut_size, int64_t ts_lo, int64_t ts_hi, int64_t n,
    unsigned long long* best_key, hipStream_t stream) {
  hipLaunchKernelGGL(series_last_ts_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream,
      ts, series, slot_lut, lut_size, ts_lo, ts_hi, n, best_key);
}

void gdb_hip::launch_prom_range_eval(
    const int64_t* ts, const double* vals, const int64_t* seg_lo,
    const int64_t* seg_hi, int S, int T, int64_t t0, int64_t step_ms,
    int64_t range_ms, int64_t offset_ms, double param, int mode, double* out,
    hipStream_t stream) {
  const int64_t total = (int64_t)S * T;
  hipLaunchKernelGGL(prom_range_eval_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream,
      ts, vals, seg_lo, seg_hi, S, T, t0, step_ms, range_ms, offset_ms,
      param, mode, out);
}

void gdb_hip::launch_series_last_row(
    const int64_t* ts, const int32_t* series, const int32_t* slot_lut,
    int lut_size, int64_t ts_lo, int64_t ts_hi, int64_t n,
    const unsigned long long* best_key, unsigned long long src_tag,
    unsigned long long* best_row, hipStream_t stream) {
  hipLaunchKernelGGL(series_last_row_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream,
      ts, series, slot_lut, lut_size, ts_lo, ts_hi, n, best_key, src_tag, best_row);
}

void gdb_hip::launch_bucket_cells(
    const int64_t* ts, const int32_t* series, const int32_t* slot_lut,
    int lut_size, int64_t ts_lo, int64_t ts_hi, int64_t origin,
    int64_t bucket_ms, int n_buckets, int64_t n, int32_t* cell,
    hipStream_t stream) {
  hipLaunchKernelGGL(bucket_cell_coalesced_kernel,
      dim3(grid_for(n, 256)), dim3(256), 0, stream,
      ts, series, slot_lut, lut_size, ts_lo, ts_hi, origin, bucket_ms,
      n_buckets, n, cell);
}

void gdb_hip::launch_quantile_hist(
    const int32_t* cell, const double* fields, int64_t field_stride,
    const int32_t* field_idx, int n_field_rows, const int32_t* field_of_sel,
    int Q, int64_t n, int n_cells, int pass, int lds_cap,
    const unsigned long long* prefix, unsigned int* hist, hipStream_t stream) {
  lds_cap = min(lds_cap, QSEL_LDS_CELLS);
  hipLaunchKernelGGL(quantile_hist_kernel, dim3(qsel_grid(n)), dim3(QSEL_BLOCK),
      0, stream, cell, fields, field_stride, field_idx, n_field_rows,
      field_of_sel, Q, n, n_cells, pass, lds_cap, prefix, hist);
}

void gdb_hip::launch_quantile_pick(
    unsigned int* hist, const double* p_of_sel, int n_cells, int64_t QC,
    int pass, unsigned long long* prefix, int64_t* k_left, int64_t* k1,
    int64_t* cnt, hipStream_t stream) {
  const int64_t blocks = (QC + 3) / 4;           // 4 wavefronts per block
  const int grid = (int)max(min(blocks, (int64_t)65536), (int64_t)1);
  hipLaunchKernelGGL(quantile_pick_kernel, dim3(grid), dim3(QSEL_BLOCK), 0,
      stream, hist, p_of_sel, n_cells, QC, pass, prefix, k_left, k1, cnt);
}

void gdb_hip::launch_quantile_next(
    const int32_t* cell, const double* fields, int64_t field_stride,
    const int32_t* field_idx, int n_field_rows, const int32_t* field_of_sel,
    int Q, int64_t n, int n_cells, int lds_cap, const unsigned long long* prefix,
    unsigned long long* le, unsigned long long* next, hipStream_t stream) {
  lds_cap = min(lds_cap, QSEL_LDS_CELLS);
  hipLaunchKernelGGL(quantile_next_kernel, dim3(qsel_grid(n)), dim3(QSEL_BLOCK),
      0, stream, cell, fields, field_stride, field_idx, n_field_rows,
      field_of_sel, Q, n, n_cells, lds_cap, prefix, le, next);
}

void gdb_hip::launch_quantile_finish(
    const unsigned long long* prefix, const int64_t* k1, const int64_t* cnt,
    const unsigned long long* le, const unsigned long long* next, int64_t QC,
    double* out_lo, double* out_hi, hipStream_t stream) {
  hipLaunchKernelGGL(quantile_finish_kernel, dim3(grid_for(QC, 256)), dim3(256),
      0, stream, prefix, k1, cnt, le, next, QC, out_lo, out_hi);
}

void gdb_hip::launch_moments_sums(
    const int32_t* cell, const double* fields, int64_t field_stride,
    const int32_t* field_idx, int n_field_rows, const int32_t* fx_of_sel,
    const int32_t* fy_of_sel, int M, int64_t n, int n_cells, int lds_cap,
    unsigned long long* cnt, double* sx, double* sy,
    unsigned long long* minx, unsigned long long* maxx,
    unsigned long long* miny, unsigned long long* maxy, hipStream_t stream) {
  lds_cap = min(lds_cap, LDS_CELLS);
  hipLaunchKernelGGL(moments_sums_kernel, dim3(moments_grid(n)), dim3(256), 0,
      stream, cell, fields, field_stride, field_idx, n_field_rows, fx_of_sel,
      fy_of_sel, M, n, n_cells, lds_cap, cnt, sx, sy, minx, maxx, miny, maxy);
}

void gdb_hip::launch_moments_mean(
    const unsigned long long* cnt, const double* sx, const double* sy,
    const unsigned long long* minx, const unsigned long long* maxx,
    const unsigned long long* miny, const unsigned long long* maxy,
    const int32_t* fx_of_sel, const int32_t* fy_of_sel, int n_cells,
    int64_t MC, double* mean_x, double* mean_y, bool* const_x, bool* const_y,
    hipStream_t stream) {
  hipLaunchKernelGGL(moments_mean_kernel, dim3(grid_for(MC, 256)), dim3(256),
      0, stream, cnt, sx, sy, minx, maxx, miny, maxy, fx_of_sel, fy_of_sel,
      n_cells, MC, mean_x, mean_y, const_x, const_y);
}

void gdb_hip::launch_moments_centred(
    const int32_t* cell, const double* fields, int64_t field_stride,
    const int32_t* field_idx, int n_field_rows, const int32_t* fx_of_sel,
    const int32_t* fy_of_sel, int M, int64_t n, int n_cells, int lds_cap,
    const double* mean_x, const double* mean_y, double* m2x, double* m2y,
    double* cxy, hipStream_t stream) {
  lds_cap = min(lds_cap, LDS_CELLS);
  hipLaunchKernelGGL(moments_centred_kernel, dim3(moments_grid(n)), dim3(256),
      0, stream, cell, fields, field_stride, field_idx, n_field_rows,
      fx_of_sel, fy_of_sel, M, n, n_cells, lds_cap, mean_x, mean_y, m2x, m2y,
      cxy);
}

void gdb_hip::launch_rle_expand_indices(
    const int64_t* runs, int64_t R, const uint8_t* blob, int bw,
    int32_t* out, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(rle_expand_indices_kernel, dim3(grid_for(n, 256)),
                     dim3(256), 0, stream, runs, R, blob, bw, out, n);
}

void gdb_hip::launch_gorilla_decode(
    const uint8_t* blob, const int64_t* block_off, const int64_t* out_off,
    int64_t B, int64_t* out_ts, double* out_val, int64_t n,
    hipStream_t stream) {
  hipLaunchKernelGGL(gorilla_decode_kernel, dim3(grid_for(n, 256)),
                     dim3(256), 0, stream, blob, block_off, out_off, B,
                     out_ts, out_val, n);
}

void gdb_hip::launch_gorilla_scale(const double* vals, int64_t n,
                                   unsigned* fail, hipStream_t stream) {
  hipLaunchKernelGGL(gorilla_scale_kernel, dim3(grid_for(n, GENC_THREADS)),
                     dim3(GENC_THREADS), 0, stream, vals, n, fail);
}

void gdb_hip::launch_gorilla_widths(
    const int64_t* ts, const double* vals, int64_t n, int block, int pack_ts,
    const unsigned* fail, uint8_t* bits, int64_t* sizes, int64_t B,
    hipStream_t stream) {
  hipLaunchKernelGGL(gorilla_widths_kernel, dim3((unsigned)B),
                     dim3(GENC_THREADS), 0, stream, ts, vals, n, block,
                     pack_ts, fail, bits, sizes);
}

void gdb_hip::launch_gorilla_write(
    const int64_t* ts, const double* vals, int64_t n, int block,
    const unsigned* fail, const uint8_t* bits, const int64_t* block_off,
    uint8_t* blob, int64_t B, hipStream_t stream) {
  hipLaunchKernelGGL(gorilla_write_kernel, dim3((unsigned)B),
                     dim3(GENC_THREADS), 0, stream, ts, vals, n, block, fail,
                     bits, block_off, blob);
}
