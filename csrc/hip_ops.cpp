// Torch bindings for greptimedb_amd._hip_ops (see kernels.hip).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <tuple>
#include <vector>

#include "kernels.h"

// The one argument check of every op below: `t` must be on the GPU and on the
// device of the op's first tensor `first`, of dtype `dt`, and contiguous.
// Like every check in this file it looks at metadata only: it reads no device
// memory and does not synchronize, so an invalid call raises before anything
// is queued and a valid call costs nothing on the device.
static void check_arg(const torch::Tensor& t, const char* name,
                      torch::ScalarType dt, const torch::Tensor& first) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.device() == first.device(), name, " is on ", t.device(),
              ", the op's first tensor on ", first.device());
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// The 5 raw accumulators of ts_bucket_agg: sum f64, cnt, min keys, max keys
// i64, each [nf, n_slots, n_buckets], and rows i64[n_slots, n_buckets].
static void check_acc(const std::vector<torch::Tensor>& acc,
                      const torch::Tensor& first) {
  TORCH_CHECK(acc.size() == 5, "acc must be the 5 raw accumulators");
  check_arg(acc[0], "acc[0] (sum)", torch::kFloat64, first);
  check_arg(acc[1], "acc[1] (cnt)", torch::kInt64, first);
  check_arg(acc[2], "acc[2] (min keys)", torch::kInt64, first);
  check_arg(acc[3], "acc[3] (max keys)", torch::kInt64, first);
  check_arg(acc[4], "acc[4] (rows)", torch::kInt64, first);
  TORCH_CHECK(acc[0].dim() == 3 && acc[4].dim() == 2 &&
              acc[1].sizes() == acc[0].sizes() &&
              acc[2].sizes() == acc[0].sizes() &&
              acc[3].sizes() == acc[0].sizes() &&
              acc[4].sizes() == acc[0].sizes().slice(1),
              "acc must be four [nf, n_slots, n_buckets] tensors and one "
              "[n_slots, n_buckets]");
}

// Fused filter + time-bucket aggregate (K1+K2+K5).
// ts: i64[n] (ms), series: i32[n], fields: f64[nf_total, field_stride]
// field_idx: i32[nf] rows of `fields` to aggregate, slot_lut: i32[lut_size].
// Returns (sum f64, count i64, min f64, max f64), each [nf, n_slots, n_buckets].
// When `acc` (5 tensors from a prior call) is passed, accumulation continues
// into the same buffers — multi-source scans make ONE set of outputs with no
// per-source combine (atomics make cross-launch accumulation safe).
std::vector<torch::Tensor> ts_bucket_agg(
    torch::Tensor ts, torch::Tensor series, torch::Tensor fields,
    torch::Tensor field_idx, torch::Tensor slot_lut,
    int64_t ts_lo, int64_t ts_hi, int64_t origin, int64_t bucket_ms,
    int64_t n_slots, int64_t n_buckets,
    std::vector<torch::Tensor> acc) {
  check_arg(ts, "ts", torch::kInt64, ts);
  check_arg(series, "series", torch::kInt32, ts);
  check_arg(fields, "fields", torch::kFloat64, ts);
  check_arg(field_idx, "field_idx", torch::kInt32, ts);
  check_arg(slot_lut, "slot_lut", torch::kInt32, ts);
  TORCH_CHECK(fields.dim() == 2);
  const int64_t n = ts.numel();
  TORCH_CHECK(series.numel() == n, "series and ts differ in length");
  TORCH_CHECK(fields.size(1) >= n, "fields stride shorter than rows");
  // cell ids are int32 and per-field offsets int in the kernels
  const int64_t nf64 = field_idx.numel();
  TORCH_CHECK(n_slots >= 0 && n_slots <= INT32_MAX && n_buckets >= 0 &&
              n_buckets <= INT32_MAX && nf64 <= INT32_MAX &&
              n_slots * n_buckets <= INT32_MAX &&
              nf64 * (n_slots * n_buckets) <= INT32_MAX,
              "nf * n_slots * n_buckets = ", nf64, " * ", n_slots, " * ",
              n_buckets, " does not fit the kernels' int32 cell arithmetic");
  const int nf = (int)nf64;
  auto opts_f64 = ts.options().dtype(torch::kFloat64);
  auto opts_i64 = ts.options().dtype(torch::kInt64);
  torch::Tensor sum, cnt, rows, minmax_init_min, minmax_init_max;
  if (!acc.empty()) {
    // what this op itself would have created below, on the same device
    check_acc(acc, ts);
    TORCH_CHECK(acc[0].size(0) == nf && acc[0].size(1) == n_slots &&
                acc[0].size(2) == n_buckets,
                "acc was made for another nf, n_slots or n_buckets");
    sum = acc[0]; cnt = acc[1]; minmax_init_min = acc[2];
    minmax_init_max = acc[3]; rows = acc[4];
  } else {
    sum = torch::zeros({nf, n_slots, n_buckets}, opts_f64);
    cnt = torch::zeros({nf, n_slots, n_buckets}, opts_i64);
    rows = torch::zeros({n_slots, n_buckets}, opts_i64);
    // min keys init to u64 max, max keys to 0
    minmax_init_min = torch::full({nf, n_slots, n_buckets}, -1, opts_i64);
    minmax_init_max = torch::zeros({nf, n_slots, n_buckets}, opts_i64);
  }
  // an empty source contributes nothing: hand back the (possibly passed-in)
  // accumulators without a launch (a zero-row launch has a zero-sized grid)
  if (n == 0) return {sum, cnt, minmax_init_min, minmax_init_max, rows};
  auto stream = at::cuda::getCurrentHIPStream().stream();
  auto cell = torch::empty({n}, ts.options().dtype(torch::kInt32));
  gdb_hip::launch_ts_bucket_agg(
      ts.data_ptr<int64_t>(), series.data_ptr<int32_t>(), fields.data_ptr<double>(),
      fields.size(1), field_idx.data_ptr<int32_t>(), nf,
      slot_lut.data_ptr<int32_t>(), (int)slot_lut.numel(),
      ts_lo, ts_hi, origin, bucket_ms, (int)n_slots, (int)n_buckets, n,
      cell.data_ptr<int32_t>(),
      sum.data_ptr<double>(),
      reinterpret_cast<unsigned long long*>(cnt.data_ptr<int64_t>()),
      reinterpret_cast<unsigned long long*>(minmax_init_min.data_ptr<int64_t>()),
      reinterpret_cast<unsigned long long*>(minmax_init_max.data_ptr<int64_t>()),
      reinterpret_cast<unsigned long long*>(rows.data_ptr<int64_t>()),
      stream);
  return {sum, cnt, minmax_init_min, minmax_init_max, rows};
}

// Decode raw accumulators (min/max u64 keys) → final (sum, cnt, min f64,
// max f64, rows). Call once after the last ts_bucket_agg of a scan.
std::vector<torch::Tensor> ts_bucket_agg_finish(std::vector<torch::Tensor> acc) {
  TORCH_CHECK(!acc.empty(), "acc must be the 5 raw accumulators");
  check_acc(acc, acc[0]);
  auto sum = acc[0];
  auto cnt = acc[1];
  const int64_t cells = cnt.numel();
  auto minv = torch::empty_like(sum);
  auto maxv = torch::empty_like(sum);
  auto stream = at::cuda::getCurrentHIPStream().stream();
  gdb_hip::launch_decode_minmax(
      reinterpret_cast<unsigned long long*>(acc[2].data_ptr<int64_t>()),
      reinterpret_cast<unsigned long long*>(acc[3].data_ptr<int64_t>()),
      reinterpret_cast<unsigned long long*>(cnt.data_ptr<int64_t>()),
      minv.data_ptr<double>(), maxv.data_ptr<double>(), cells, stream);
  return {sum, cnt, minv, maxv, acc[4]};
}

torch::Tensor filter_series_time(
    torch::Tensor ts, torch::Tensor series, torch::Tensor slot_lut,
    int64_t ts_lo, int64_t ts_hi) {
  check_arg(ts, "ts", torch::kInt64, ts);
  check_arg(series, "series", torch::kInt32, ts);
  const int64_t n = ts.numel();
  auto keep = torch::empty({n}, ts.options().dtype(torch::kBool));
  // an empty LUT selects every series; the kernel then never reads `series`
  const int32_t* lut = nullptr;
  int lut_size = 0;
  if (slot_lut.numel() > 0) {
    check_arg(slot_lut, "slot_lut", torch::kInt32, ts);
    TORCH_CHECK(series.numel() == n, "series and ts differ in length");
    lut = slot_lut.data_ptr<int32_t>();
    lut_size = (int)slot_lut.numel();
  }
  auto stream = at::cuda::getCurrentHIPStream().stream();
  gdb_hip::launch_filter_series_time(
      ts.data_ptr<int64_t>(), series.data_ptr<int32_t>(), lut, lut_size,
      ts_lo, ts_hi, n, keep.data_ptr<bool>(), stream);
  return keep;
}

torch::Tensor dedup_mark_last(torch::Tensor series, torch::Tensor ts) {
  check_arg(series, "series", torch::kInt32, series);
  check_arg(ts, "ts", torch::kInt64, series);
  const int64_t n = ts.numel();
  TORCH_CHECK(series.numel() == n, "series and ts differ in length");
  auto keep = torch::empty({n}, ts.options().dtype(torch::kBool));
  auto stream = at::cuda::getCurrentHIPStream().stream();
  gdb_hip::launch_dedup_mark_last(
      series.data_ptr<int32_t>(), ts.data_ptr<int64_t>(), n,
      keep.data_ptr<bool>(), stream);
  return keep;
}

// last_non_null merge over (series, ts, seq)-sorted rows: kidx i64[g] = the
// last row of every (series, ts) group, merged f64[nf, g] = per field the
// newest non-NaN value of the group (the last row's bits if there is none).
// The group count is data dependent, so nonzero() reads it back, as the
// LastRow path's own nonzero does.
std::tuple<torch::Tensor, torch::Tensor> merge_last_non_null(
    torch::Tensor series, torch::Tensor ts, torch::Tensor fields) {
  check_arg(series, "series", torch::kInt32, series);
  check_arg(ts, "ts", torch::kInt64, series);
  check_arg(fields, "fields", torch::kFloat64, series);
  TORCH_CHECK(fields.dim() == 2);
  const int64_t n = ts.numel();
  const int64_t nf = fields.size(0);
  TORCH_CHECK(series.numel() == n);
  TORCH_CHECK(fields.size(1) == n, "fields must be [nf, n]");
  auto opts_f64 = ts.options().dtype(torch::kFloat64);
  if (n == 0)
    return {torch::empty({0}, ts.options().dtype(torch::kInt64)),
            torch::empty({nf, 0}, opts_f64)};
  auto kidx = dedup_mark_last(series, ts).nonzero().reshape({-1});
  const int64_t g = kidx.numel();
  auto merged = torch::empty({nf, g}, opts_f64);
  if (nf == 0) return {kidx, merged};
  auto stream = at::cuda::getCurrentHIPStream().stream();
  gdb_hip::launch_merge_last_non_null(
      kidx.data_ptr<int64_t>(), g, fields.data_ptr<double>(), n, (int)nf,
      merged.data_ptr<double>(), stream);
  return {kidx, merged};
}

// Arguments the two lastpoint ops share. best_key and best_row are indexed by
// the slots that slot_lut holds on the device, so their length against the
// LUT's values stays the caller's contract (ops.series_last sizes them).
static void check_lastpoint_args(const torch::Tensor& ts,
                                 const torch::Tensor& series,
                                 const torch::Tensor& slot_lut,
                                 const torch::Tensor& best_key) {
  check_arg(ts, "ts", torch::kInt64, ts);
  check_arg(series, "series", torch::kInt32, ts);
  check_arg(slot_lut, "slot_lut", torch::kInt32, ts);
  check_arg(best_key, "best_key", torch::kInt64, ts);
  TORCH_CHECK(series.numel() == ts.numel(), "series and ts differ in length");
}

// Accumulate per-slot max-ts keys across sources (call once per source with
// a shared best_key tensor, int64 viewed as u64 keys, init 0).
void series_last_ts(torch::Tensor ts, torch::Tensor series, torch::Tensor slot_lut,
                    int64_t ts_lo, int64_t ts_hi, torch::Tensor best_key) {
  check_lastpoint_args(ts, series, slot_lut, best_key);
  auto stream = at::cuda::getCurrentHIPStream().stream();
  gdb_hip::launch_series_last(
      ts.data_ptr<int64_t>(), series.data_ptr<int32_t>(),
      slot_lut.data_ptr<int32_t>(), (int)slot_lut.numel(), ts_lo, ts_hi,
      ts.numel(),
      reinterpret_cast<unsigned long long*>(best_key.data_ptr<int64_t>()),
      stream);
}

void series_last_row(torch::Tensor ts, torch::Tensor series, torch::Tensor slot_lut,
                     int64_t ts_lo, int64_t ts_hi, torch::Tensor best_key,
                     int64_t src_tag, torch::Tensor best_row) {
  check_lastpoint_args(ts, series, slot_lut, best_key);
  check_arg(best_row, "best_row", torch::kInt64, ts);
  auto stream = at::cuda::getCurrentHIPStream().stream();
  gdb_hip::launch_series_last_row(
      ts.data_ptr<int64_t>(), series.data_ptr<int32_t>(),
      slot_lut.data_ptr<int32_t>(), (int)slot_lut.numel(), ts_lo, ts_hi,
      ts.numel(),
      reinterpret_cast<const unsigned long long*>(best_key.data_ptr<int64_t>()),
      (unsigned long long)src_tag,
      reinterpret_cast<unsigned long long*>(best_row.data_ptr<int64_t>()),
      stream);
}

// PromQL range/instant evaluation over (slot, ts)-sorted samples.
torch::Tensor prom_range_eval(
    torch::Tensor ts, torch::Tensor vals, torch::Tensor seg_lo, torch::Tensor seg_hi,
    int64_t T, int64_t t0, int64_t step_ms, int64_t range_ms, int64_t offset_ms,
    double param, int64_t mode) {
  check_arg(ts, "ts", torch::kInt64, ts);
  check_arg(vals, "vals", torch::kFloat64, ts);
  check_arg(seg_lo, "seg_lo", torch::kInt64, ts);
  check_arg(seg_hi, "seg_hi", torch::kInt64, ts);
  TORCH_CHECK(vals.numel() == ts.numel(), "vals and ts differ in length");
  TORCH_CHECK(seg_hi.numel() == seg_lo.numel(),
              "seg_lo and seg_hi differ in length");
  // the segment bounds themselves live on the device: 0 <= seg_lo <= seg_hi
  // <= ts.numel() is the caller's contract
  const int S = (int)seg_lo.numel();
  auto out = torch::empty({S, T}, vals.options());
  auto stream = at::cuda::getCurrentHIPStream().stream();
  gdb_hip::launch_prom_range_eval(
      ts.data_ptr<int64_t>(), vals.data_ptr<double>(),
      seg_lo.data_ptr<int64_t>(), seg_hi.data_ptr<int64_t>(),
      S, (int)T, t0, step_ms, range_ms, offset_ms, param, (int)mode,
      out.data_ptr<double>(), stream);
  return out;
}

// K16 bulk append: scatter one routed batch into multiple region memtables.
// `dests` = per-region (ts, series, fields) destination tensors.
void scatter_append(
    torch::Tensor ts, torch::Tensor series, torch::Tensor fields,
    torch::Tensor region_of, torch::Tensor dst_off,
    std::vector<torch::Tensor> dst_ts, std::vector<torch::Tensor> dst_se,
    std::vector<torch::Tensor> dst_fields) {
  check_arg(ts, "ts", torch::kInt64, ts);
  check_arg(series, "series", torch::kInt32, ts);
  check_arg(fields, "fields", torch::kFloat64, ts);
  check_arg(region_of, "region_of", torch::kInt32, ts);
  check_arg(dst_off, "dst_off", torch::kInt64, ts);
  const int64_t n = ts.numel();
  TORCH_CHECK(fields.dim() == 2 && fields.size(1) == n, "fields must be [nf, n]");
  TORCH_CHECK(series.numel() == n && region_of.numel() == n &&
              dst_off.numel() == n,
              "series, region_of and dst_off must have one element per row");
  const int nf = (int)fields.size(0);
  const int R = (int)dst_ts.size();
  TORCH_CHECK(dst_se.size() == dst_ts.size() &&
              dst_fields.size() == dst_ts.size(),
              "per-region lists differ in length");
  // The VALUES of region_of and dst_off live on the device and are not read
  // back: 0 <= region_of[i] < R and a dst_off[i] inside region region_of[i]
  // are the caller's contract (scatter_append_packed checks them on the host
  // because its batch starts there).
  std::vector<int64_t> hptrs(R * 3 + R);
  for (int r = 0; r < R; r++) {
    check_arg(dst_ts[r], "dst_ts[r]", torch::kInt64, ts);
    check_arg(dst_se[r], "dst_se[r]", torch::kInt32, ts);
    check_arg(dst_fields[r], "dst_fields[r]", torch::kFloat64, ts);
    TORCH_CHECK(dst_fields[r].dim() == 2 && dst_fields[r].size(0) >= nf,
                "region ", r, " has fewer field rows than the batch");
    hptrs[r] = (int64_t)dst_ts[r].data_ptr<int64_t>();
    hptrs[R + r] = (int64_t)dst_se[r].data_ptr<int32_t>();
    hptrs[2 * R + r] = (int64_t)dst_fields[r].data_ptr<double>();
    hptrs[3 * R + r] = dst_fields[r].size(1);  // stride = cap
  }
  auto ptrs = torch::from_blob(hptrs.data(), {(int64_t)hptrs.size()},
                               torch::kInt64).to(ts.device());
  auto stream = at::cuda::getCurrentHIPStream().stream();
  const int64_t* pbase = ptrs.data_ptr<int64_t>();
  gdb_hip::launch_scatter_append(
      ts.data_ptr<int64_t>(), series.data_ptr<int32_t>(),
      fields.data_ptr<double>(), region_of.data_ptr<int32_t>(),
      dst_off.data_ptr<int64_t>(),
      reinterpret_cast<int64_t* const*>(pbase),
      reinterpret_cast<int32_t* const*>(pbase + R),
      reinterpret_cast<double* const*>(pbase + 2 * R),
      pbase + 3 * R, nf, n, stream);
}

// K16, packed form: upload one routed batch with ONE non-blocking copy of
// the used prefix of a pinned host block, then scatter it into the region
// memtables with one launch; destinations go by value as kernel arguments.
// Block layout (8-byte aligned segments, see csrc/ingest_core.h):
//   ts i64[n] | fields f64[nf*n] | dst_off i64[n] | series i32[n] | region i32[n]
// Row i lands at bases[region[i]] + dst_off[i]. Copy and kernel run on the
// current stream; the caller must not refill `stage_pinned` before work
// queued here has finished (it records an event after this call).
void scatter_append_packed(
    torch::Tensor stage_pinned, torch::Tensor stage_dev, int64_t n, int64_t nf,
    std::vector<int64_t> bases, std::vector<torch::Tensor> dst_ts,
    std::vector<torch::Tensor> dst_se, std::vector<torch::Tensor> dst_fields) {
  TORCH_CHECK(!stage_pinned.is_cuda() && stage_pinned.is_pinned(),
              "stage_pinned must be pinned host memory");
  check_arg(stage_dev, "stage_dev", torch::kUInt8, stage_dev);
  TORCH_CHECK(stage_pinned.is_contiguous() &&
              stage_pinned.scalar_type() == torch::kUInt8,
              "stage_pinned must be contiguous uint8");
  TORCH_CHECK(n >= 0 && nf >= 0);
  if (n == 0) return;
  const int R = (int)dst_ts.size();
  TORCH_CHECK(R >= 1 && R <= gdb_hip::kPackedRegions,
              "scatter_append_packed handles 1..16 regions, got ", R);
  TORCH_CHECK((int)bases.size() == R && (int)dst_se.size() == R &&
              (int)dst_fields.size() == R, "per-region lists differ in length");
  const int64_t i32_bytes = (4 * n + 7) & ~(int64_t)7;
  const int64_t off_dst = 8 * n + 8 * nf * n;
  const int64_t off_region = off_dst + 8 * n + i32_bytes;
  const int64_t used = off_region + i32_bytes;
  TORCH_CHECK(used <= stage_pinned.numel() && used <= stage_dev.numel(),
              "stage block smaller than the batch");
  gdb_hip::PackedRegions regs;
  std::vector<int64_t> room(R);
  for (int r = 0; r < gdb_hip::kPackedRegions; r++) {
    regs.ts[r] = nullptr; regs.se[r] = nullptr; regs.f[r] = nullptr;
    regs.stride[r] = 0; regs.base[r] = 0;
  }
  for (int r = 0; r < R; r++) {
    check_arg(dst_ts[r], "dst_ts[r]", torch::kInt64, stage_dev);
    check_arg(dst_se[r], "dst_se[r]", torch::kInt32, stage_dev);
    check_arg(dst_fields[r], "dst_fields[r]", torch::kFloat64, stage_dev);
    TORCH_CHECK(dst_fields[r].dim() == 2 && dst_fields[r].size(0) >= nf,
                "region ", r, " has fewer field rows than the batch");
    TORCH_CHECK(bases[r] >= 0);
    regs.ts[r] = dst_ts[r].data_ptr<int64_t>();
    regs.se[r] = dst_se[r].data_ptr<int32_t>();
    regs.f[r] = dst_fields[r].data_ptr<double>();
    regs.stride[r] = dst_fields[r].size(1);
    regs.base[r] = bases[r];
    room[r] = std::min(std::min(dst_ts[r].numel(), dst_se[r].numel()),
                       dst_fields[r].size(1));
  }
  // every destination row is checked on the host before anything is queued
  const uint8_t* hp = stage_pinned.data_ptr<uint8_t>();
  const int64_t* h_dst = reinterpret_cast<const int64_t*>(hp + off_dst);
  const int32_t* h_region = reinterpret_cast<const int32_t*>(hp + off_region);
  for (int64_t i = 0; i < n; i++) {
    const int32_t r = h_region[i];
    TORCH_CHECK(r >= 0 && r < R, "row ", i, ": region ", r, " out of range");
    TORCH_CHECK(h_dst[i] >= 0 && bases[r] + h_dst[i] < room[r],
                "row ", i, ": destination row beyond region ", r, " capacity");
  }
  auto stream = at::cuda::getCurrentHIPStream().stream();
  uint8_t* dp = stage_dev.data_ptr<uint8_t>();
  // Everything above ran under the GIL; from here on only raw pointers and
  // plain values are touched, so the copy and the launch are queued with the
  // GIL released: other ingest workers run their Python sections meanwhile.
  hipError_t err = hipSuccess, lerr = hipSuccess;
  {
    py::gil_scoped_release nogil;
    err = hipMemcpyAsync(dp, hp, (size_t)used, hipMemcpyHostToDevice, stream);
    if (err == hipSuccess) {
      gdb_hip::launch_scatter_append_packed(dp, n, (int)nf, regs, stream);
      lerr = hipGetLastError();
    }
  }
  TORCH_CHECK(err == hipSuccess, "stage upload failed: ", hipGetErrorString(err));
  TORCH_CHECK(lerr == hipSuccess, "scatter_append_packed launch failed: ",
              hipGetErrorString(lerr));
}

// K11: parquet hybrid RLE/bit-packed dictionary indices → i32 on device.
// runs: i64[R,5] (host-built, csrc/pagedec.cpp), blob: u8 device tensor
// (pad >= 8 bytes past the last packed bit).
torch::Tensor rle_expand_indices(torch::Tensor runs, torch::Tensor blob,
                                 int64_t bw, int64_t n) {
  check_arg(runs, "runs", torch::kInt64, runs);
  check_arg(blob, "blob", torch::kUInt8, runs);
  TORCH_CHECK(runs.dim() == 2 && runs.size(1) == 5, "runs must be [R, 5]");
  TORCH_CHECK(bw >= 1 && bw <= 32, "bw must be in [1, 32], got ", bw);
  TORCH_CHECK(n == 0 || runs.size(0) >= 1, "no runs for ", n, " values");
  // the run table's offsets and counts live on the device: runs that cover
  // [0, n) and stay inside the padded blob are the caller's contract
  auto out = torch::empty({n}, blob.options().dtype(torch::kInt32));
  auto stream = at::cuda::getCurrentHIPStream().stream();
  gdb_hip::launch_rle_expand_indices(
      runs.data_ptr<int64_t>(), runs.size(0), blob.data_ptr<uint8_t>(),
      (int)bw, out.data_ptr<int32_t>(), n, stream);
  return out;
}

// K20: Gorilla/delta block decode → (ts i64[n], vals f64[n]) on device.
std::vector<torch::Tensor> gorilla_decode(torch::Tensor blob,
                                          torch::Tensor block_off,
                                          torch::Tensor out_off, int64_t n) {
  check_arg(blob, "blob", torch::kUInt8, blob);
  check_arg(block_off, "block_off", torch::kInt64, blob);
  check_arg(out_off, "out_off", torch::kInt64, blob);
  TORCH_CHECK(out_off.numel() == block_off.numel(),
              "block_off and out_off differ in length");
  TORCH_CHECK(n == 0 || block_off.numel() >= 1, "no blocks for ", n, " values");
  auto ts = torch::empty({n}, blob.options().dtype(torch::kInt64));
  auto vals = torch::empty({n}, blob.options().dtype(torch::kFloat64));
  auto stream = at::cuda::getCurrentHIPStream().stream();
  gdb_hip::launch_gorilla_decode(
      blob.data_ptr<uint8_t>(), block_off.data_ptr<int64_t>(),
      out_off.data_ptr<int64_t>(), block_off.numel(),
      ts.data_ptr<int64_t>(), vals.data_ptr<double>(), n, stream);
  return {ts, vals};
}

// K20: Gorilla/delta block encode on device → (blob u8, block_off i64[B],
// out_off i64[B]), byte for byte what engine/gorilla.py pack() returns.
// `vals` None packs like a column of zeros (the ts-only pack). One
// device-to-host read (the total size) sizes the blob.
std::vector<torch::Tensor> gorilla_encode(torch::Tensor ts,
                                          c10::optional<torch::Tensor> vals,
                                          int64_t block, bool pack_ts) {
  check_arg(ts, "ts", torch::kInt64, ts);
  TORCH_CHECK(ts.dim() == 1, "ts must be one-dimensional");
  TORCH_CHECK(block >= 1 && block <= gdb_hip::GENC_MAX_BLOCK,
              "gorilla_encode: block must be in [1, ", gdb_hip::GENC_MAX_BLOCK,
              "], got ", block);
  const int64_t n = ts.numel();
  const double* vals_p = nullptr;
  if (vals.has_value()) {
    const torch::Tensor& v = *vals;
    check_arg(v, "vals", torch::kFloat64, ts);
    TORCH_CHECK(v.dim() == 1 && v.numel() == n, "vals must match ts in length");
    vals_p = v.data_ptr<double>();
  }
  auto opts_u8 = ts.options().dtype(torch::kUInt8);
  auto opts_i64 = ts.options().dtype(torch::kInt64);
  const int64_t B = (n + block - 1) / block;
  TORCH_CHECK(B <= INT32_MAX, "gorilla_encode: too many blocks");
  if (B == 0)
    return {torch::zeros({16}, opts_u8), torch::empty({0}, opts_i64),
            torch::empty({0}, opts_i64)};
  auto stream = at::cuda::getCurrentHIPStream().stream();
  auto fail = torch::zeros({1}, ts.options().dtype(torch::kInt32));
  auto* fail_p = reinterpret_cast<unsigned*>(fail.data_ptr<int32_t>());
  if (vals_p != nullptr)
    gdb_hip::launch_gorilla_scale(vals_p, n, fail_p, stream);
  auto bits = torch::empty({B, 2}, opts_u8);
  auto sizes = torch::empty({B}, opts_i64);
  gdb_hip::launch_gorilla_widths(
      ts.data_ptr<int64_t>(), vals_p, n, (int)block, pack_ts ? 1 : 0, fail_p,
      bits.data_ptr<uint8_t>(), sizes.data_ptr<int64_t>(), B, stream);
  auto ends = torch::cumsum(sizes, 0);
  auto block_off = ends - sizes;
  const int64_t total = ends[B - 1].item<int64_t>() + 16;
  auto blob = torch::zeros({total}, opts_u8);
  gdb_hip::launch_gorilla_write(
      ts.data_ptr<int64_t>(), vals_p, n, (int)block, fail_p,
      bits.data_ptr<uint8_t>(), block_off.data_ptr<int64_t>(),
      blob.data_ptr<uint8_t>(), B, stream);
  auto out_off = torch::arange(B, opts_i64) * block;
  return {blob, block_off, out_off};
}

// Phase A of the bucket aggregate on its own: the (slot, bucket) cell id of
// every row, slot * n_buckets + bucket, or -1 where the row is filtered out.
torch::Tensor bucket_cells(
    torch::Tensor ts, torch::Tensor series, torch::Tensor slot_lut,
    int64_t ts_lo, int64_t ts_hi, int64_t origin, int64_t bucket_ms,
    int64_t n_buckets) {
  check_arg(ts, "ts", torch::kInt64, ts);
  check_arg(series, "series", torch::kInt32, ts);
  check_arg(slot_lut, "slot_lut", torch::kInt32, ts);
  TORCH_CHECK(bucket_ms > 0 && n_buckets > 0 && n_buckets <= INT32_MAX);
  const int64_t n = ts.numel();
  TORCH_CHECK(series.numel() == n);
  auto cell = torch::empty({n}, ts.options().dtype(torch::kInt32));
  if (n == 0) return cell;
  auto stream = at::cuda::getCurrentHIPStream().stream();
  gdb_hip::launch_bucket_cells(
      ts.data_ptr<int64_t>(), series.data_ptr<int32_t>(),
      slot_lut.data_ptr<int32_t>(), (int)slot_lut.numel(), ts_lo, ts_hi,
      origin, bucket_ms, (int)n_buckets, n, cell.data_ptr<int32_t>(), stream);
  return cell;
}

// One (cell i32[n], fields f64[nf_total, >=n], field_idx i32[nf]) source of
// the grouped ops below, against the first source's cell tensor.
static void check_cell_source(const torch::Tensor& cell,
                              const torch::Tensor& fields,
                              const torch::Tensor& fidx,
                              const torch::Tensor& first) {
  check_arg(cell, "cell", torch::kInt32, first);
  check_arg(fidx, "field_idx", torch::kInt32, first);
  TORCH_CHECK(cell.dim() == 1 && fidx.dim() == 1);
  // fields may be a row-strided view (a memtable's used prefix), so it is
  // the one tensor that does not go through check_arg
  TORCH_CHECK(fields.is_cuda() && fields.device() == first.device(),
              "fields must be a GPU tensor on the first source's device");
  TORCH_CHECK(fields.scalar_type() == torch::kFloat64 && fields.dim() == 2);
  TORCH_CHECK(fields.size(1) >= cell.numel(), "fields shorter than rows");
  TORCH_CHECK(fields.size(1) <= 1 || fields.stride(1) == 1,
              "fields must have unit stride along rows");
  TORCH_CHECK(fields.size(0) <= 1 || fields.stride(0) >= fields.size(1),
              "fields rows overlap");
}

// Exact grouped order statistics (K21). sources: (cell i32[n], fields
// f64[nf_total, >=n] with unit inner stride, field_idx i32[nf]) triples that
// accumulate into one state; selection s reads field row
// field_idx[field_of_sel[s]] and looks for rank k1 = floor((cnt-1) * p[s]).
// Returns (lo, hi f64[Q, n_cells], cnt i64[Q, n_cells]): the values of rank
// k1 and min(k1+1, cnt-1) and the non-NaN count; NaN where cnt == 0.
// field_of_sel is checked against field_idx's length here; the VALUES of
// field_idx live on the device and are not read back: an entry outside
// [0, fields.size(0)) makes the kernels skip that selection for that source
// (its rows count nowhere, nothing out of bounds is touched). Callers build
// field_idx on the host from valid row positions.
// on_pass, if given, is called between the streaming passes (cancellation).
// lds_cells caps the cell span a tile may have to count in LDS (the kernels
// clamp it to their table size); 0 forces global atomics, for measurement.
static constexpr int64_t kMaxQuantileCells = 262144;   // 256 MiB of u32 bins

std::vector<torch::Tensor> grouped_quantile(
    std::vector<std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>> sources,
    std::vector<int64_t> field_of_sel, std::vector<double> p_of_sel,
    int64_t n_cells, py::object on_pass, int64_t lds_cells) {
  TORCH_CHECK(lds_cells >= 0, "lds_cells must not be negative");
  const int64_t Q = (int64_t)field_of_sel.size();
  TORCH_CHECK(Q >= 1, "grouped_quantile needs at least one selection");
  TORCH_CHECK((int64_t)p_of_sel.size() == Q, "p_of_sel and field_of_sel differ in length");
  TORCH_CHECK(n_cells >= 1, "n_cells must be positive");
  TORCH_CHECK(n_cells <= kMaxQuantileCells && Q * n_cells <= kMaxQuantileCells,
              "grouped_quantile: Q * n_cells = ", Q, " * ", n_cells,
              " exceeds ", kMaxQuantileCells);
  for (double p : p_of_sel)
    TORCH_CHECK(p >= 0.0 && p <= 1.0, "p must lie in [0, 1], got ", p);
  uint64_t total_rows = 0;
  torch::Device dev(torch::kCPU);
  for (auto& src : sources) {
    auto& cell = std::get<0>(src);
    auto& fields = std::get<1>(src);
    auto& fidx = std::get<2>(src);
    check_cell_source(cell, fields, fidx, std::get<0>(sources.front()));
    for (int64_t f : field_of_sel)
      TORCH_CHECK(f >= 0 && f < fidx.numel(), "field_of_sel ", f,
                  " outside field_idx of length ", fidx.numel());
    total_rows += (uint64_t)cell.numel();
    dev = cell.device();
  }
  TORCH_CHECK(total_rows < (1ULL << 32),
              "grouped_quantile: ", total_rows, " rows overflow the u32 bins");
  const int64_t QC = Q * n_cells;
  auto o_f64 = torch::TensorOptions().dtype(torch::kFloat64).device(dev);
  auto o_i64 = torch::TensorOptions().dtype(torch::kInt64).device(dev);
  auto cnt = torch::zeros({Q, n_cells}, o_i64);
  if (total_rows == 0) {
    auto nan = torch::full({Q, n_cells}, std::nan(""), o_f64);
    return {nan, nan.clone(), cnt};
  }
  auto o_i32 = o_i64.dtype(torch::kInt32);
  auto hist = torch::zeros({QC, 256}, o_i32);
  auto prefix = torch::zeros({QC}, o_i64);
  auto k_left = torch::zeros({QC}, o_i64);
  auto k1 = torch::zeros({QC}, o_i64);
  auto le = torch::zeros({QC}, o_i64);
  auto next = torch::full({QC}, -1, o_i64);            // u64 max = "no next"
  std::vector<int32_t> fos32(field_of_sel.begin(), field_of_sel.end());
  auto fos = torch::from_blob(fos32.data(), {Q}, torch::kInt32).to(dev);
  auto ps = torch::from_blob(p_of_sel.data(), {Q}, torch::kFloat64).to(dev);
  auto stream = at::cuda::getCurrentHIPStream().stream();
  auto* prefix_p = reinterpret_cast<unsigned long long*>(prefix.data_ptr<int64_t>());
  auto* hist_p = reinterpret_cast<unsigned int*>(hist.data_ptr<int32_t>());
  auto* le_p = reinterpret_cast<unsigned long long*>(le.data_ptr<int64_t>());
  auto* next_p = reinterpret_cast<unsigned long long*>(next.data_ptr<int64_t>());
  auto check = [](const char* what) {
    const hipError_t err = hipGetLastError();
    TORCH_CHECK(err == hipSuccess, what, " launch failed: ", hipGetErrorString(err));
  };
  auto between = [&]() { if (!on_pass.is_none()) on_pass(); };
  auto field_stride = [](const torch::Tensor& f) {
    return f.size(0) > 1 ? f.stride(0) : f.size(1);
  };
  for (int pass = 0; pass < 8; pass++) {
    for (auto& src : sources) {
      auto& cell = std::get<0>(src);
      auto& fields = std::get<1>(src);
      auto& fidx = std::get<2>(src);
      if (cell.numel() == 0) continue;
      gdb_hip::launch_quantile_hist(
          cell.data_ptr<int32_t>(), fields.data_ptr<double>(), field_stride(fields),
          fidx.data_ptr<int32_t>(), (int)fields.size(0), fos.data_ptr<int32_t>(),
          (int)Q, cell.numel(), (int)n_cells, pass, (int)std::min<int64_t>(lds_cells, 1 << 20),
          prefix_p, hist_p, stream);
      check("quantile_hist");
    }
    gdb_hip::launch_quantile_pick(
        hist_p, ps.data_ptr<double>(), (int)n_cells, QC, pass, prefix_p,
        k_left.data_ptr<int64_t>(), k1.data_ptr<int64_t>(),
        cnt.data_ptr<int64_t>(), stream);
    check("quantile_pick");
    between();
  }
  for (auto& src : sources) {
    auto& cell = std::get<0>(src);
    auto& fields = std::get<1>(src);
    auto& fidx = std::get<2>(src);
    if (cell.numel() == 0) continue;
    gdb_hip::launch_quantile_next(
        cell.data_ptr<int32_t>(), fields.data_ptr<double>(), field_stride(fields),
        fidx.data_ptr<int32_t>(), (int)fields.size(0), fos.data_ptr<int32_t>(),
        (int)Q, cell.numel(), (int)n_cells, (int)std::min<int64_t>(lds_cells, 1 << 20),
        prefix_p, le_p, next_p, stream);
    check("quantile_next");
  }
  auto lo = torch::empty({Q, n_cells}, o_f64);
  auto hi = torch::empty({Q, n_cells}, o_f64);
  gdb_hip::launch_quantile_finish(
      prefix_p, k1.data_ptr<int64_t>(), cnt.data_ptr<int64_t>(), le_p, next_p,
      QC, lo.data_ptr<double>(), hi.data_ptr<double>(), stream);
  check("quantile_finish");
  return {lo, hi, cnt};
}

// Grouped second moments (K22) in two passes with no host synchronisation.
// sources as for grouped_quantile; selection s pairs field rows
// field_idx[fx_of_sel[s]] and field_idx[fy_of_sel[s]] (fx == fy: one column).
// A row counts in its cell where neither value is NaN. Returns, each
// [M, n_cells]: n i64, mean_x, mean_y, m2x, m2y, cxy f64, const_x, const_y
// bool. m2 = sum (x - mean)^2 and cxy = sum (x - mean_x)(y - mean_y) over
// the counted rows; const = min == max over them, and then m2 (and cxy) is
// exactly 0. n == 0: NaN means, zero sums, flags clear. As in
// grouped_quantile, a field_idx VALUE outside fields makes the kernels skip
// that selection for that source. lds_cells caps the cell span a tile may
// have to accumulate in LDS (clamped to LDS_CELLS); 0 forces global atomics.
std::vector<torch::Tensor> grouped_moments(
    std::vector<std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>> sources,
    std::vector<int64_t> fx_of_sel, std::vector<int64_t> fy_of_sel,
    int64_t n_cells, int64_t lds_cells) {
  TORCH_CHECK(lds_cells >= 0, "lds_cells must not be negative");
  const int64_t M = (int64_t)fx_of_sel.size();
  TORCH_CHECK(M >= 1, "grouped_moments needs at least one selection");
  TORCH_CHECK((int64_t)fy_of_sel.size() == M, "fx_of_sel and fy_of_sel differ in length");
  TORCH_CHECK(n_cells >= 1, "n_cells must be positive");
  TORCH_CHECK(n_cells <= kMaxQuantileCells && M * n_cells <= kMaxQuantileCells,
              "grouped_moments: M * n_cells = ", M, " * ", n_cells,
              " exceeds ", kMaxQuantileCells);
  int64_t total_rows = 0;
  torch::Device dev(torch::kCPU);
  for (auto& src : sources) {
    auto& cell = std::get<0>(src);
    auto& fidx = std::get<2>(src);
    check_cell_source(cell, std::get<1>(src), fidx, std::get<0>(sources.front()));
    for (int64_t s = 0; s < M; s++)
      TORCH_CHECK(fx_of_sel[s] >= 0 && fx_of_sel[s] < fidx.numel() &&
                  fy_of_sel[s] >= 0 && fy_of_sel[s] < fidx.numel(),
                  "selection (", fx_of_sel[s], ", ", fy_of_sel[s],
                  ") outside field_idx of length ", fidx.numel());
    total_rows += cell.numel();
    dev = cell.device();
  }
  TORCH_CHECK(sources.empty() || dev.is_cuda());
  if (sources.empty()) dev = torch::Device(torch::kCUDA, at::cuda::current_device());
  auto o_f64 = torch::TensorOptions().dtype(torch::kFloat64).device(dev);
  auto o_i64 = o_f64.dtype(torch::kInt64);
  auto o_bool = o_f64.dtype(torch::kBool);
  auto cnt = torch::zeros({M, n_cells}, o_i64);
  auto m2x = torch::zeros({M, n_cells}, o_f64);
  auto m2y = torch::zeros({M, n_cells}, o_f64);
  auto cxy = torch::zeros({M, n_cells}, o_f64);
  if (total_rows == 0) {
    auto nan = torch::full({M, n_cells}, std::nan(""), o_f64);
    auto no = torch::zeros({M, n_cells}, o_bool);
    return {cnt, nan, nan.clone(), m2x, m2y, cxy, no, no.clone()};
  }
  auto sx = torch::zeros({M, n_cells}, o_f64);
  auto sy = torch::zeros({M, n_cells}, o_f64);
  auto minx = torch::full({M, n_cells}, -1, o_i64);     // u64 max
  auto maxx = torch::zeros({M, n_cells}, o_i64);
  auto miny = torch::full({M, n_cells}, -1, o_i64);
  auto maxy = torch::zeros({M, n_cells}, o_i64);
  auto mean_x = torch::empty({M, n_cells}, o_f64);
  auto mean_y = torch::empty({M, n_cells}, o_f64);
  auto const_x = torch::empty({M, n_cells}, o_bool);
  auto const_y = torch::empty({M, n_cells}, o_bool);
  std::vector<int32_t> sel32(2 * M);
  std::vector<int64_t> same;                    // selections with x == y
  for (int64_t s = 0; s < M; s++) {
    sel32[s] = (int32_t)fx_of_sel[s];
    sel32[M + s] = (int32_t)fy_of_sel[s];
    if (fx_of_sel[s] == fy_of_sel[s]) same.push_back(s);
  }
  auto sel_d = torch::from_blob(sel32.data(), {2 * M}, torch::kInt32).to(dev);
  const int32_t* fx_p = sel_d.data_ptr<int32_t>();
  const int32_t* fy_p = fx_p + M;
  auto stream = at::cuda::getCurrentHIPStream().stream();
  auto u64 = [](torch::Tensor& t) {
    return reinterpret_cast<unsigned long long*>(t.data_ptr<int64_t>());
  };
  auto check = [](const char* what) {
    const hipError_t err = hipGetLastError();
    TORCH_CHECK(err == hipSuccess, what, " launch failed: ", hipGetErrorString(err));
  };
  auto field_stride = [](const torch::Tensor& f) {
    return f.size(0) > 1 ? f.stride(0) : f.size(1);
  };
  const int lds_cap = (int)std::min<int64_t>(lds_cells, gdb_hip::LDS_CELLS);
  for (auto& src : sources) {
    auto& cell = std::get<0>(src);
    auto& fields = std::get<1>(src);
    auto& fidx = std::get<2>(src);
    if (cell.numel() == 0) continue;
    gdb_hip::launch_moments_sums(
        cell.data_ptr<int32_t>(), fields.data_ptr<double>(), field_stride(fields),
        fidx.data_ptr<int32_t>(), (int)fields.size(0), fx_p, fy_p, (int)M,
        cell.numel(), (int)n_cells, lds_cap, u64(cnt), sx.data_ptr<double>(),
        sy.data_ptr<double>(), u64(minx), u64(maxx), u64(miny), u64(maxy),
        stream);
    check("moments_sums");
  }
  gdb_hip::launch_moments_mean(
      u64(cnt), sx.data_ptr<double>(), sy.data_ptr<double>(), u64(minx),
      u64(maxx), u64(miny), u64(maxy), fx_p, fy_p, (int)n_cells, M * n_cells,
      mean_x.data_ptr<double>(), mean_y.data_ptr<double>(),
      const_x.data_ptr<bool>(), const_y.data_ptr<bool>(), stream);
  check("moments_mean");
  for (auto& src : sources) {
    auto& cell = std::get<0>(src);
    auto& fields = std::get<1>(src);
    auto& fidx = std::get<2>(src);
    if (cell.numel() == 0) continue;
    gdb_hip::launch_moments_centred(
        cell.data_ptr<int32_t>(), fields.data_ptr<double>(), field_stride(fields),
        fidx.data_ptr<int32_t>(), (int)fields.size(0), fx_p, fy_p, (int)M,
        cell.numel(), (int)n_cells, lds_cap, mean_x.data_ptr<double>(),
        mean_y.data_ptr<double>(), m2x.data_ptr<double>(),
        m2y.data_ptr<double>(), cxy.data_ptr<double>(), stream);
    check("moments_centred");
  }
  // one-argument selections filled only the x planes
  if (!same.empty()) {
    auto idx = torch::from_blob(same.data(), {(int64_t)same.size()}, torch::kInt64).to(dev);
    auto one = m2x.index_select(0, idx);
    m2y.index_copy_(0, idx, one);
    cxy.index_copy_(0, idx, one);
  }
  // a constant column has x - mean == 0 in every row unless it is infinite
  m2x.masked_fill_(const_x, 0.0);
  m2y.masked_fill_(const_y, 0.0);
  cxy.masked_fill_(const_x.logical_or(const_y), 0.0);
  return {cnt, mean_x, mean_y, m2x, m2y, cxy, const_x, const_y};
}

// {tile rows, LDS cell capacity, grid cap} of the selection kernels.
std::vector<int64_t> quantile_launch_config() {
  return {gdb_hip::QSEL_TILE, gdb_hip::QSEL_LDS_CELLS, gdb_hip::QSEL_MAX_GRID};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  // geometry of the bucket aggregate, for tests that build tiles at its edges
  m.attr("AGG_TILE") = gdb_hip::AGG_TILE;
  m.attr("LDS_CELLS") = gdb_hip::LDS_CELLS;
  m.def("ts_bucket_agg", &ts_bucket_agg, "fused filter + time-bucket aggregate",
        py::arg("ts"), py::arg("series"), py::arg("fields"), py::arg("field_idx"),
        py::arg("slot_lut"), py::arg("ts_lo"), py::arg("ts_hi"), py::arg("origin"),
        py::arg("bucket_ms"), py::arg("n_slots"), py::arg("n_buckets"),
        py::arg("acc") = std::vector<torch::Tensor>());
  m.def("ts_bucket_agg_finish", &ts_bucket_agg_finish, "decode raw accumulators");
  m.def("rle_expand_indices", &rle_expand_indices, "K11 hybrid RLE expand");
  m.def("gorilla_decode", &gorilla_decode, "K20 gorilla block decode");
  m.def("gorilla_encode", &gorilla_encode, "K20 gorilla block encode",
        py::arg("ts"), py::arg("vals"), py::arg("block"), py::arg("pack_ts"));
  m.def("filter_series_time", &filter_series_time, "series/time filter mask");
  m.def("dedup_mark_last", &dedup_mark_last, "last-row dedup marker");
  m.def("merge_last_non_null", &merge_last_non_null,
        "last_non_null merge: (group-last rows, merged fields)");
  m.def("series_last_ts", &series_last_ts, "per-slot max-ts accumulate (lastpoint)");
  m.def("series_last_row", &series_last_row, "per-slot winner row (lastpoint)");
  m.def("prom_range_eval", &prom_range_eval, "PromQL range-vector evaluator");
  m.def("scatter_append", &scatter_append, "bulk routed memtable append (K16)");
  m.def("scatter_append_packed", &scatter_append_packed,
        "K16 from one packed pinned block: one H2D copy + one launch");
  m.def("bucket_cells", &bucket_cells, "(slot, bucket) cell id per row",
        py::arg("ts"), py::arg("series"), py::arg("slot_lut"), py::arg("ts_lo"),
        py::arg("ts_hi"), py::arg("origin"), py::arg("bucket_ms"),
        py::arg("n_buckets"));
  m.def("grouped_quantile", &grouped_quantile,
        "exact grouped order statistics by radix-histogram selection (K21)",
        py::arg("sources"), py::arg("field_of_sel"), py::arg("p_of_sel"),
        py::arg("n_cells"), py::arg("on_pass") = py::none(),
        py::arg("lds_cells") = 16);
  m.def("grouped_moments", &grouped_moments,
        "grouped variance / covariance planes in two passes (K22)",
        py::arg("sources"), py::arg("fx_of_sel"), py::arg("fy_of_sel"),
        py::arg("n_cells"), py::arg("lds_cells") = gdb_hip::LDS_CELLS);
  m.def("quantile_launch_config", &quantile_launch_config,
        "tile rows, LDS cell capacity and grid cap of the selection kernels");
}
