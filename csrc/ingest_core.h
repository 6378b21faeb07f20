// Line-protocol parse + route core of the ingest path. Header-only and free
// of any Python dependency, so it compiles into greptimedb_amd._native
// (csrc/native.cpp holds the pybind glue) and into the stand-alone checker
// csrc/ingest_core_check.cpp that runs it under host sanitizers.
//
//  LineCore      influx line protocol → columnar batch, written straight into
//                caller-chosen destination columns (ParseSink). Tagsets and
//                field names are interned through a flat open-addressing
//                table keyed by a word-at-a-time hash.
//  fused_ingest  parse + route + WAL payload build for the steady-state
//                single-table batch: the row data lands in ONE packed block
//                (`stage`, see StageLayout) that the device path uploads with
//                a single copy.

#pragma once

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

namespace gdb_ingest {

// ------------------------------------------------------------------ hashing

static inline uint64_t load64(const char* p) {
  uint64_t v;
  std::memcpy(&v, p, 8);
  return v;
}

static inline uint64_t mix64(uint64_t a, uint64_t b) {
  const __uint128_t r = (__uint128_t)a * b;
  return (uint64_t)r ^ (uint64_t)(r >> 64);
}

// 64-bit hash over a byte range, 8 bytes per load, two independent
// multiply-fold lanes per 32-byte block (a ~230-byte series key is 8 folds
// deep instead of 230 dependent multiplies). Process-internal: never stored.
static inline uint64_t hash64(const char* p, size_t n) {
  const uint64_t K0 = 0x9E3779B97F4A7C15ULL, K1 = 0xA0761D6478BD642FULL,
                 K2 = 0xE7037ED1A0B428DBULL;
  const char* const end = p + n;
  uint64_t s0 = K0 ^ n, s1 = K2;
  size_t left = n;
  while (left >= 32) {
    s0 = mix64(load64(p) ^ K1, load64(p + 8) ^ s0);
    s1 = mix64(load64(p + 16) ^ K2, load64(p + 24) ^ s1);
    p += 32;
    left -= 32;
  }
  if (left >= 16) {
    s0 = mix64(load64(p) ^ K1, load64(p + 8) ^ s0);
    p += 16;
    left -= 16;
  }
  uint64_t a = 0, b = 0;
  if (n >= 16) {              // last 16 bytes (may overlap what was folded)
    a = load64(end - 16);
    b = load64(end - 8);
  } else if (n >= 8) {
    a = load64(end - n);
    b = load64(end - 8);
  } else if (n > 0) {
    std::memcpy(&a, end - n, n);
  }
  return mix64(K1 ^ n, mix64(a ^ K1, b ^ s0 ^ s1));
}

// Open-addressing (linear probe) hash → id table. The caller verifies the
// bytes behind a candidate id, so equal hashes of different keys coexist.
class FlatTable {
 public:
  FlatTable() { slots_.assign(1024, Slot{0, -1}); }

  template <class Eq>
  int32_t find(uint64_t h, Eq eq) const {
    const size_t mask = slots_.size() - 1;
    for (size_t i = (size_t)h & mask;; i = (i + 1) & mask) {
      const Slot& s = slots_[i];
      if (s.id < 0) return -1;
      if (s.h == h && eq(s.id)) return s.id;
    }
  }

  void insert(uint64_t h, int32_t id) {
    if ((count_ + 1) * 10 > slots_.size() * 7) grow();
    place(slots_, h, id);
    count_++;
  }

  size_t size() const { return count_; }
  size_t capacity() const { return slots_.size(); }

 private:
  struct Slot {
    uint64_t h;
    int32_t id;
  };
  static void place(std::vector<Slot>& slots, uint64_t h, int32_t id) {
    const size_t mask = slots.size() - 1;
    size_t i = (size_t)h & mask;
    while (slots[i].id >= 0) i = (i + 1) & mask;
    slots[i] = Slot{h, id};
  }
  void grow() {
    std::vector<Slot> bigger(slots_.size() * 2, Slot{0, -1});
    for (const Slot& s : slots_)
      if (s.id >= 0) place(bigger, s.h, s.id);
    slots_.swap(bigger);
  }
  std::vector<Slot> slots_;
  size_t count_ = 0;
};

// ------------------------------------------------------------ value parsing

// Fast decimal parse for the common "[-]digits[.digits]" shape; falls back to
// strtod for exponents/inf/nan.
static inline double fast_atof(const char* p, const char* end) {
  bool neg = false;
  const char* s = p;
  if (s < end && (*s == '-' || *s == '+')) { neg = (*s == '-'); s++; }
  uint64_t ip = 0; int nd = 0;
  while (s < end && *s >= '0' && *s <= '9' && nd < 18) { ip = ip * 10 + (*s - '0'); s++; nd++; }
  double v = (double)ip;
  if (s < end && *s == '.') {
    s++;
    uint64_t fp = 0; int fd = 0;
    while (s < end && *s >= '0' && *s <= '9' && fd < 18) { fp = fp * 10 + (*s - '0'); s++; fd++; }
    static const double pow10[19] = {1e0,1e1,1e2,1e3,1e4,1e5,1e6,1e7,1e8,1e9,1e10,
                                     1e11,1e12,1e13,1e14,1e15,1e16,1e17,1e18};
    v += (double)fp / pow10[fd];
  }
  if (s < end && (*s == 'e' || *s == 'E')) return strtod(p, nullptr);  // rare
  return neg ? -v : v;
}

static inline int64_t fast_atoll(const char* p, const char* end) {
  bool neg = false;
  if (p < end && (*p == '-' || *p == '+')) { neg = (*p == '-'); p++; }
  int64_t v = 0;
  while (p < end && *p >= '0' && *p <= '9') { v = v * 10 + (*p - '0'); p++; }
  return neg ? -v : v;
}

// --------------------------------------------------------------- LineCore

// Where one parse writes. `series`/`ts` and every `col[c]` have room for
// `cap` rows (cap >= LineCore::count_lines of the batch). col[c] is the
// destination of parser field c; fields first seen during the parse get a
// NaN-prefilled column in `extra` (col[c] points into it).
struct ParseSink {
  int32_t* series = nullptr;
  int64_t* ts = nullptr;
  size_t cap = 0;
  std::vector<double*> col;
  std::vector<std::vector<double>> extra;
  std::vector<std::pair<int32_t, std::string>> new_tagsets;
};

class LineCore {
 public:
  // Lines that parse() will look at (non-empty, not a '#' comment): an upper
  // bound of the row count, exact unless a line is malformed.
  static size_t count_lines(const char* buf, size_t len) {
    size_t rows = 0;
    const char* p = buf;
    const char* end = buf + len;
    while (p < end) {
      const char* nl = static_cast<const char*>(std::memchr(p, '\n', end - p));
      const char* line_end = nl ? nl : end;
      if (line_end > p && *p != '#') rows++;
      p = nl ? nl + 1 : end;
    }
    return rows;
  }

  // Parse a batch into `s`; returns the row count. Every column in s.col is
  // fully written for rows [0, n): absent fields become NaN.
  size_t parse(const char* buf, size_t len, ParseSink& s) {
    if (stamp_.size() < field_names_.size()) stamp_.resize(field_names_.size(), 0);
    size_t nrows = 0;
    const char* p = buf;
    const char* end = buf + len;
    while (p < end) {
      const char* nl = static_cast<const char*>(std::memchr(p, '\n', end - p));
      const char* line_end = nl ? nl : end;
      if (line_end > p && *p != '#') parse_line(p, line_end, s, nrows);
      p = nl ? nl + 1 : end;
    }
    return nrows;
  }

  size_t num_series() const { return tagset_ids_.size(); }
  size_t num_fields() const { return field_names_.size(); }
  const std::vector<std::string>& field_names() const { return field_names_; }
  size_t intern_capacity() const { return tagset_ids_.capacity(); }

  const std::string* tagset_str(int32_t sid) const {
    if (sid < 0 || (size_t)sid >= tagset_strs_.size()) return nullptr;
    return &tagset_strs_[sid];
  }

  // Restore dictionary state (e.g. after WAL replay / reopen).
  void register_tagset(const std::string& s, int32_t id) {
    tagset_ids_.insert(hash64(s.data(), s.size()), id);
    if (tagset_strs_.size() < (size_t)id + 1) tagset_strs_.resize((size_t)id + 1);
    tagset_strs_[id] = s;
    if (next_id_ < id + 1) next_id_ = id + 1;
  }
  void register_field(const std::string& name) { field_idx(name.data(), name.size()); }

 private:
  void parse_line(const char* p, const char* end, ParseSink& r, size_t& nrows) {
    // measurement,tagset fieldset [timestamp]
    // NOTE: influx escape sequences (\,, \ , \=) are not handled — TSBS and
    // our writers never emit them.
    const char* sp1 = static_cast<const char*>(std::memchr(p, ' ', end - p));
    if (!sp1) return;  // malformed
    const char* sp2 = static_cast<const char*>(std::memchr(sp1 + 1, ' ', end - sp1 - 1));

    // series key = "measurement,tagset" — interned via hash probe + byte
    // verify (no per-row allocation on the hit path)
    const size_t klen = sp1 - p;
    const uint64_t h = hash64(p, klen);
    int32_t sid = tagset_ids_.find(h, [&](int32_t id) {
      const std::string& s = tagset_strs_[id];
      return s.size() == klen && std::memcmp(s.data(), p, klen) == 0;
    });
    if (sid < 0) {
      sid = next_id_++;
      tagset_ids_.insert(h, sid);
      if (tagset_strs_.size() < (size_t)sid + 1) tagset_strs_.resize((size_t)sid + 1);
      tagset_strs_[sid].assign(p, klen);
      r.new_tagsets.emplace_back(sid, tagset_strs_[sid]);
    }

    // timestamp (ns); missing timestamp → 0 (caller fills server time)
    int64_t tsv = 0;
    if (sp2) tsv = fast_atoll(sp2 + 1, end);

    const size_t row = nrows++;
    r.series[row] = sid;
    r.ts[row] = tsv;

    // fieldset: k=v,k=v,...
    const uint64_t row_stamp = ++stamp_ctr_;
    size_t nset = 0;
    const char* f = sp1 + 1;
    const char* fend = sp2 ? sp2 : end;
    size_t fpos = 0;
    while (f < fend) {
      const char* eq = static_cast<const char*>(std::memchr(f, '=', fend - f));
      if (!eq) break;
      const char* comma = static_cast<const char*>(std::memchr(eq + 1, ',', fend - eq - 1));
      const char* vend = comma ? comma : fend;
      double val;
      const char* v = eq + 1;
      if (v < vend && (*v == '"')) {
        // string field value — not representable in the float column; store NaN.
        val = std::nan("");
      } else if (vend > v && (vend[-1] == 'i' || vend[-1] == 'u')) {
        val = static_cast<double>(fast_atoll(v, vend - 1));
      } else if (vend > v && (*v == 't' || *v == 'T' || *v == 'f' || *v == 'F')) {
        val = (*v == 't' || *v == 'T') ? 1.0 : 0.0;
      } else {
        val = fast_atof(v, vend);
      }
      // positional field cache: batches of lines share a fieldset layout
      // (TSBS and most collectors), so field j of each row is usually the
      // same name — memcmp against the cached name skips hash+probe
      size_t c;
      const size_t flen = eq - f;
      if (fpos < fcache_.size() && fcache_[fpos].first == flen &&
          std::memcmp(field_names_[fcache_[fpos].second].data(), f, flen) == 0) {
        c = fcache_[fpos].second;
      } else {
        c = field_idx(f, flen);
        if (fpos >= fcache_.size()) fcache_.resize(fpos + 1);
        fcache_[fpos] = {flen, c};
      }
      fpos++;
      if (c >= r.col.size()) {       // field first seen in this batch
        while (r.col.size() <= c) {
          r.extra.emplace_back(r.cap, std::nan(""));
          r.col.push_back(r.extra.back().data());
        }
      }
      if (c >= stamp_.size()) stamp_.resize(c + 1, 0);
      if (stamp_[c] != row_stamp) { stamp_[c] = row_stamp; nset++; }
      r.col[c][row] = val;
      f = comma ? comma + 1 : fend;
    }
    if (nset != r.col.size()) {      // row lacks some field: NaN it
      const double nan = std::nan("");
      for (size_t c = 0; c < r.col.size(); c++)
        if (c >= stamp_.size() || stamp_[c] != row_stamp) r.col[c][row] = nan;
    }
  }

  size_t field_idx(const char* name, size_t len) {
    const uint64_t h = hash64(name, len);
    const int32_t hit = fmap_.find(h, [&](int32_t id) {
      const std::string& s = field_names_[id];
      return s.size() == len && std::memcmp(s.data(), name, len) == 0;
    });
    if (hit >= 0) return (size_t)hit;
    const size_t idx = field_names_.size();
    fmap_.insert(h, (int32_t)idx);
    field_names_.emplace_back(name, len);
    return idx;
  }

  FlatTable tagset_ids_;
  std::vector<std::string> tagset_strs_;
  int32_t next_id_ = 0;
  FlatTable fmap_;
  std::vector<std::string> field_names_;
  std::vector<std::pair<size_t, size_t>> fcache_;  // positional (len, idx)
  std::vector<uint64_t> stamp_;   // per field: stamp of the last row that set it
  uint64_t stamp_ctr_ = 0;
};

// ------------------------------------------------------------ fused ingest

static inline size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

// Packed row block of one routed batch; every segment 8-byte aligned:
//   ts i64[n] | fields f64[nf*n] (row-major, table order) | dst_off i64[n]
//   | series i32[n] | region i32[n]
// The device kernel (csrc/kernels.hip) derives the same offsets from (n, nf).
struct StageLayout {
  size_t ts, fields, dst_off, series, region, total;
  StageLayout(size_t n, size_t nf) {
    ts = 0;
    fields = 8 * n;
    dst_off = fields + 8 * nf * n;
    series = dst_off + 8 * n;
    region = series + align8(4 * n);
    total = region + align8(4 * n);
  }
};

constexpr int kMaxPackedRegions = 16;   // kernel-argument region table size

enum FusedStatus { FUSED_OK = 0, FUSED_SLOW = 1, FUSED_GROW = 2 };

struct FusedResult {
  FusedStatus status = FUSED_SLOW;
  size_t n = 0;            // rows
  size_t need_bytes = 0;   // FUSED_GROW: stage size this batch needs
  // FUSED_OK: per-region row count, min/max ts (ms) and WAL payloads
  // (payload r = wal[wal_off[r] .. wal_off[r+1]), empty when count is 0)
  std::vector<int64_t> counts, mins, maxs;
  std::vector<char> wal;
  std::vector<size_t> wal_off;
  // FUSED_SLOW: the ordinary parse result in parser field order. sink.series,
  // sink.ts and sink.col point into `stage` or into the owned buffers below.
  ParseSink sink;
  std::vector<int32_t> own_series;
  std::vector<int64_t> own_ts;
  std::vector<double> own_cols;
};

// Parse `buf`, then — when every row belongs to a routed series of the one
// table the LUTs describe — route it: series codes, ts in ms, per-row region
// and destination offset, table-ordered fields and the per-region WAL
// payloads (wal.encode_batch layout), all in one pass with no Python.
//   sid_region[sid]  table-local region index of parser series sid, -1 when
//                    the series is new, unrouted, remote or of another table
//   sid_local[sid]   region-local series code
//   fmap[t]          parser field index of table field t, -1 = absent (NaN)
//   n_parser_fields  parser field count fmap was built for
// Anything else is FUSED_SLOW: the caller continues on the general path with
// the parse result (the batch is never parsed twice).
static inline void fused_ingest(
    LineCore& core, const char* buf, size_t len,
    const int32_t* sid_region, const int32_t* sid_local, size_t lut_len,
    const int64_t* fmap, int nf, size_t n_parser_fields, int n_regions,
    const std::string& hdr_suffix, bool durable, int64_t ts_scale,
    char* stage, size_t stage_bytes, FusedResult& out) {
  const size_t est = LineCore::count_lines(buf, len);
  const size_t F = core.num_fields();
  bool direct = lut_len > 0 && n_regions > 0 && n_regions <= kMaxPackedRegions &&
                n_parser_fields == F && est > 0;
  if (direct) {
    for (int t = 0; t < nf; t++)
      if (fmap[t] >= (int64_t)F) direct = false;
  }
  if (direct) {
    const StageLayout need(est, (size_t)nf);
    if (need.total > stage_bytes) {
      out.status = FUSED_GROW;
      out.need_bytes = need.total;
      return;
    }
  }
  ParseSink& sink = out.sink;
  sink.cap = est;
  sink.col.assign(F, nullptr);
  const StageLayout L(est, (size_t)nf);
  if (direct) {
    sink.ts = reinterpret_cast<int64_t*>(stage + L.ts);
    sink.series = reinterpret_cast<int32_t*>(stage + L.series);
    double* fblock = reinterpret_cast<double*>(stage + L.fields);
    for (int t = 0; t < nf; t++)
      if (fmap[t] >= 0) sink.col[fmap[t]] = fblock + (size_t)t * est;
    // parser fields the table does not carry still need somewhere to land
    for (size_t c = 0; c < F; c++) {
      if (sink.col[c] == nullptr) {
        sink.extra.emplace_back(est, std::nan(""));
        sink.col[c] = sink.extra.back().data();
      }
    }
  } else {
    out.own_series.resize(est);
    out.own_ts.resize(est);
    out.own_cols.resize(F * est);
    sink.series = out.own_series.data();
    sink.ts = out.own_ts.data();
    for (size_t c = 0; c < F; c++) sink.col[c] = out.own_cols.data() + c * est;
  }
  const size_t n = core.parse(buf, len, sink);
  out.n = n;
  out.status = FUSED_SLOW;
  if (!direct || n == 0) {
    if (n == 0 && sink.new_tagsets.empty() && core.num_fields() == F)
      out.status = FUSED_OK;    // nothing to write
    return;
  }
  if (core.num_fields() != F || !sink.new_tagsets.empty()) return;
  for (size_t i = 0; i < n; i++) {
    const int32_t sid = sink.series[i];
    if (sid < 0 || (size_t)sid >= lut_len) return;
    const int32_t r = sid_region[sid];
    if (r < 0 || r >= n_regions) return;
  }

  // ---- fast path: from here on the stage block is converted in place
  const StageLayout P(n, (size_t)nf);
  if (n != est) {   // malformed lines were dropped: close the gaps
    // every segment moves towards the block start, lowest address first
    const double* src = reinterpret_cast<const double*>(stage + L.fields);
    double* dst = reinterpret_cast<double*>(stage + P.fields);
    for (int t = 0; t < nf; t++)
      std::memmove(dst + (size_t)t * n, src + (size_t)t * est, 8 * n);
    std::memmove(stage + P.series, stage + L.series, 4 * n);
  }
  int64_t* ts = reinterpret_cast<int64_t*>(stage + P.ts);
  double* fields = reinterpret_cast<double*>(stage + P.fields);
  int64_t* dst_off = reinterpret_cast<int64_t*>(stage + P.dst_off);
  int32_t* series = reinterpret_cast<int32_t*>(stage + P.series);
  int32_t* region = reinterpret_cast<int32_t*>(stage + P.region);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int t = 0; t < nf; t++)
    if (fmap[t] < 0)
      for (size_t i = 0; i < n; i++) fields[(size_t)t * n + i] = nan;

  out.counts.assign(n_regions, 0);
  out.mins.assign(n_regions, INT64_MAX);
  out.maxs.assign(n_regions, INT64_MIN);
  int64_t* cnt = out.counts.data();
  int64_t* mn = out.mins.data();
  int64_t* mx = out.maxs.data();
  for (size_t i = 0; i < n; i++) {
    const int32_t sid = series[i];
    const int32_t r = sid_region[sid];
    series[i] = sid_local[sid];
    region[i] = r;
    dst_off[i] = cnt[r]++;
    // ts_ns * scale wraps like the int64 array product it replaces; the
    // division floors (python //), also for negative timestamps
    const int64_t t_ns = (int64_t)((uint64_t)ts[i] * (uint64_t)ts_scale);
    int64_t t = t_ns / 1000000;
    if (t_ns % 1000000 < 0) t--;
    ts[i] = t;
    if (t < mn[r]) mn[r] = t;
    if (t > mx[r]) mx[r] = t;
  }
  out.status = FUSED_OK;
  out.wal_off.assign((size_t)n_regions + 1, 0);
  if (!durable) return;

  // per-region WAL payloads: [u32 hdr_len][hdr json][i32 codes][i64 ts]
  // [f64 fields nf*m], exactly wal.encode_batch; hdr_suffix is the cached
  // json tail after the value of "n"
  std::vector<std::string> hdrs(n_regions);
  std::vector<size_t> code_off(n_regions), ts_off(n_regions), f_off(n_regions);
  size_t total = 0;
  for (int r = 0; r < n_regions; r++) {
    out.wal_off[r] = total;
    const size_t m = (size_t)cnt[r];
    if (m == 0) continue;
    hdrs[r] = "{\"n\": " + std::to_string(cnt[r]) + hdr_suffix;
    code_off[r] = total + 4 + hdrs[r].size();
    ts_off[r] = code_off[r] + 4 * m;
    f_off[r] = ts_off[r] + 8 * m;
    total = f_off[r] + 8 * (size_t)nf * m;
  }
  out.wal_off[n_regions] = total;
  out.wal.resize(total);
  char* w = out.wal.data();
  for (int r = 0; r < n_regions; r++) {
    if (cnt[r] == 0) continue;
    const uint32_t hl = (uint32_t)hdrs[r].size();
    std::memcpy(w + out.wal_off[r], &hl, 4);
    std::memcpy(w + out.wal_off[r] + 4, hdrs[r].data(), hl);
  }
  for (size_t i = 0; i < n; i++) {
    const int32_t r = region[i];
    const size_t o = (size_t)dst_off[i];
    const size_t m = (size_t)cnt[r];
    std::memcpy(w + code_off[r] + 4 * o, series + i, 4);
    std::memcpy(w + ts_off[r] + 8 * o, ts + i, 8);
    char* fdst = w + f_off[r];
    for (int t = 0; t < nf; t++)
      std::memcpy(fdst + 8 * ((size_t)t * m + o), fields + (size_t)t * n + i, 8);
  }
}

}  // namespace gdb_ingest
