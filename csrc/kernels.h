// Launch interface of the gfx950 kernels, declared once for kernels.hip (which
// defines the launchers by qualified name, so a drifted signature does not
// compile) and hip_ops.cpp (which validates arguments before calling them).
// Launchers only queue work on `stream`; pointers are device pointers.

#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace gdb_hip {

// bucket aggregate: rows per tile, cells of the LDS accumulator table
constexpr int AGG_TILE = 8192;
constexpr int LDS_CELLS = 1024;
// quantile selection: tile rows, block threads, LDS cell span, grid cap
constexpr int QSEL_TILE = 2048;
constexpr int QSEL_BLOCK = 256;
constexpr int QSEL_ROWS = QSEL_TILE / QSEL_BLOCK;
constexpr int QSEL_LDS_CELLS = 16;
constexpr int QSEL_MAX_GRID = 1024;
constexpr int GENC_MAX_BLOCK = 4096;  // Gorilla encoder: values per codec block
constexpr int kPackedRegions = 16;    // scatter_append_packed: regions per launch

// Destinations of up to kPackedRegions region memtables, passed by value:
// 5 * 16 * 8 = 640 bytes of kernel arguments, no device-side pointer table.
struct PackedRegions {
  int64_t* ts[kPackedRegions];
  int32_t* se[kPackedRegions];
  double* f[kPackedRegions];        // fields [nf, stride] row-major
  int64_t stride[kPackedRegions];   // field row stride (memtable capacity)
  int64_t base[kPackedRegions];     // first free row before this batch
};

// phase A on its own: (slot, bucket) cell id per row, -1 = filtered out
void launch_bucket_cells(
    const int64_t* ts, const int32_t* series, const int32_t* slot_lut,
    int lut_size, int64_t ts_lo, int64_t ts_hi, int64_t origin,
    int64_t bucket_ms, int n_buckets, int64_t n, int32_t* cell,
    hipStream_t stream);
// both phases; cell_buf is i32[n] scratch, n >= 1
void launch_ts_bucket_agg(
    const int64_t* ts, const int32_t* series, const double* fields,
    int64_t field_stride, const int32_t* field_idx, int nf,
    const int32_t* slot_lut, int lut_size,
    int64_t ts_lo, int64_t ts_hi, int64_t origin, int64_t bucket_ms,
    int n_slots, int n_buckets, int64_t n,
    int32_t* cell_buf,
    double* out_sum, unsigned long long* out_cnt,
    unsigned long long* out_min, unsigned long long* out_max,
    unsigned long long* out_rows, hipStream_t stream);
void launch_decode_minmax(
    const unsigned long long* minkey, const unsigned long long* maxkey,
    const unsigned long long* cnt, double* out_min, double* out_max,
    int64_t n, hipStream_t stream);

void launch_filter_series_time(
    const int64_t* ts, const int32_t* series, const int32_t* slot_lut,
    int lut_size, int64_t ts_lo, int64_t ts_hi, int64_t n, bool* keep,
    hipStream_t stream);
void launch_dedup_mark_last(
    const int32_t* series, const int64_t* ts, int64_t n, bool* keep,
    hipStream_t stream);
void launch_merge_last_non_null(
    const int64_t* kidx, int64_t g, const double* fields, int64_t field_stride,
    int nf, double* out, hipStream_t stream);

void launch_series_last(
    const int64_t* ts, const int32_t* series, const int32_t* slot_lut,
    int lut_size, int64_t ts_lo, int64_t ts_hi, int64_t n,
    unsigned long long* best_key, hipStream_t stream);
void launch_series_last_row(
    const int64_t* ts, const int32_t* series, const int32_t* slot_lut,
    int lut_size, int64_t ts_lo, int64_t ts_hi, int64_t n,
    const unsigned long long* best_key, unsigned long long src_tag,
    unsigned long long* best_row, hipStream_t stream);

void launch_prom_range_eval(
    const int64_t* ts, const double* vals, const int64_t* seg_lo,
    const int64_t* seg_hi, int S, int T, int64_t t0, int64_t step_ms,
    int64_t range_ms, int64_t offset_ms, double param, int mode, double* out,
    hipStream_t stream);

void launch_quantile_hist(
    const int32_t* cell, const double* fields, int64_t field_stride,
    const int32_t* field_idx, int n_field_rows, const int32_t* field_of_sel,
    int Q, int64_t n, int n_cells, int pass, int lds_cap,
    const unsigned long long* prefix, unsigned int* hist, hipStream_t stream);
void launch_quantile_pick(
    unsigned int* hist, const double* p_of_sel, int n_cells, int64_t QC,
    int pass, unsigned long long* prefix, int64_t* k_left, int64_t* k1,
    int64_t* cnt, hipStream_t stream);
void launch_quantile_next(
    const int32_t* cell, const double* fields, int64_t field_stride,
    const int32_t* field_idx, int n_field_rows, const int32_t* field_of_sel,
    int Q, int64_t n, int n_cells, int lds_cap, const unsigned long long* prefix,
    unsigned long long* le, unsigned long long* next, hipStream_t stream);
void launch_quantile_finish(
    const unsigned long long* prefix, const int64_t* k1, const int64_t* cnt,
    const unsigned long long* le, const unsigned long long* next, int64_t QC,
    double* out_lo, double* out_hi, hipStream_t stream);

// grouped moments: planes are [M, n_cells]; min keys start at u64 max, every
// other accumulator at 0; n >= 1; lds_cap is clamped to LDS_CELLS
void launch_moments_sums(
    const int32_t* cell, const double* fields, int64_t field_stride,
    const int32_t* field_idx, int n_field_rows, const int32_t* fx_of_sel,
    const int32_t* fy_of_sel, int M, int64_t n, int n_cells, int lds_cap,
    unsigned long long* cnt, double* sx, double* sy,
    unsigned long long* minx, unsigned long long* maxx,
    unsigned long long* miny, unsigned long long* maxy, hipStream_t stream);
void launch_moments_mean(
    const unsigned long long* cnt, const double* sx, const double* sy,
    const unsigned long long* minx, const unsigned long long* maxx,
    const unsigned long long* miny, const unsigned long long* maxy,
    const int32_t* fx_of_sel, const int32_t* fy_of_sel, int n_cells,
    int64_t MC, double* mean_x, double* mean_y, bool* const_x, bool* const_y,
    hipStream_t stream);
void launch_moments_centred(
    const int32_t* cell, const double* fields, int64_t field_stride,
    const int32_t* field_idx, int n_field_rows, const int32_t* fx_of_sel,
    const int32_t* fy_of_sel, int M, int64_t n, int n_cells, int lds_cap,
    const double* mean_x, const double* mean_y, double* m2x, double* m2y,
    double* cxy, hipStream_t stream);

void launch_scatter_append(
    const int64_t* ts, const int32_t* series, const double* fields,
    const int32_t* region_of, const int64_t* dst_off,
    int64_t* const* ts_ptrs, int32_t* const* se_ptrs, double* const* f_ptrs,
    const int64_t* strides, int nf, int64_t n, hipStream_t stream);
void launch_scatter_append_packed(
    const unsigned char* stage, int64_t n, int nf, const PackedRegions& regs,
    hipStream_t stream);

void launch_rle_expand_indices(
    const int64_t* runs, int64_t R, const uint8_t* blob, int bw,
    int32_t* out, int64_t n, hipStream_t stream);
void launch_gorilla_decode(
    const uint8_t* blob, const int64_t* block_off, const int64_t* out_off,
    int64_t B, int64_t* out_ts, double* out_val, int64_t n,
    hipStream_t stream);
// `fail` must be zeroed by the caller; `vals` may be null (no value column)
void launch_gorilla_scale(const double* vals, int64_t n, unsigned* fail,
                          hipStream_t stream);
void launch_gorilla_widths(
    const int64_t* ts, const double* vals, int64_t n, int block, int pack_ts,
    const unsigned* fail, uint8_t* bits, int64_t* sizes, int64_t B,
    hipStream_t stream);
void launch_gorilla_write(
    const int64_t* ts, const double* vals, int64_t n, int block,
    const unsigned* fail, const uint8_t* bits, const int64_t* block_off,
    uint8_t* blob, int64_t B, hipStream_t stream);

}  // namespace gdb_hip
