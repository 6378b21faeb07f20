// greptimedb_amd._native — host-side native ingest path.
//
// Two components, both on the ingest hot path:
//  1. LineParser — influx line protocol → columnar batch. Replaces the
//     reference's per-protocol row decoding (src/servers/src/influxdb.rs +
//     row protos). Tagsets are dict-encoded to dense int32 series refs with
//     an interned-string map so steady-state ingest never re-parses tags.
//  2. WalWriter — segmented group-commit WAL writer (reference:
//     src/log-store raft_engine backend + mito2 wal.rs:187 WalWriter).
//     Frame: [u32 len][u32 crc32][u64 region_id][u64 seq][payload].
//     Frame, checksum and file logic live in csrc/wal_core.h.
//
// Deliberately torch-free: compiles in seconds, usable from any process.

#include <pybind11/pybind11.h>
#include <pybind11/numpy.h>
#include <pybind11/stl.h>

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fcntl.h>
#include <stdexcept>
#include <string>
#include <unistd.h>
#include <unordered_map>
#include <vector>

#include "ingest_core.h"
#include "wal_core.h"

namespace py = pybind11;

// crc32 (IEEE, zlib-compatible): csrc/wal_core.h, carry-less-multiply
// folding where the CPU has it, slice-by-8 otherwise and for tails.
using gdb_wal::crc32_update;

// FNV-1a 64-bit over a byte range (interning probe of the prom/otlp parsers
// and the tokenizer; the line parser hashes a word at a time, ingest_core.h).
static inline uint64_t fnv1a(const char* p, size_t n) {
  uint64_t h = 1469598103934665603ULL;
  for (size_t i = 0; i < n; i++) { h ^= (uint8_t)p[i]; h *= 1099511628211ULL; }
  return h;
}

// ---------------------------------------------------------------- LineParser
// pybind glue over gdb_ingest::LineCore / fused_ingest (csrc/ingest_core.h).

// numpy array over malloc'd memory that the array (and its views) own.
static py::capsule owner_of(void* p) {
  return py::capsule(p, [](void* q) { std::free(q); });
}

class LineParser {
 public:
  // Parse a batch of lines. Returns (series i32[n], ts i64[n],
  // {field: f64[n]}, [(id, tagset_bytes)...new]). The field arrays are rows
  // of one [F, n] block the parser wrote directly.
  py::tuple parse(py::bytes data) {
    char* buf;
    Py_ssize_t len;
    if (PyBytes_AsStringAndSize(data.ptr(), &buf, &len) != 0)
      throw std::runtime_error("expected bytes");
    gdb_ingest::ParseSink sink;
    const size_t F0 = core_.num_fields();
    size_t nrows = 0, est = 0;
    int32_t* series = nullptr;
    int64_t* ts = nullptr;
    double* block = nullptr;
    {
      py::gil_scoped_release rel;  // pure C scan; enables threaded ingest workers
      est = gdb_ingest::LineCore::count_lines(buf, (size_t)len);
      series = static_cast<int32_t*>(std::malloc(4 * est + 8));
      ts = static_cast<int64_t*>(std::malloc(8 * est + 8));
      block = static_cast<double*>(std::malloc(8 * est * F0 + 8));
      if (series && ts && block) {
        sink.series = series;
        sink.ts = ts;
        sink.cap = est;
        sink.col.resize(F0);
        for (size_t c = 0; c < F0; c++) sink.col[c] = block + c * est;
        nrows = core_.parse(buf, (size_t)len, sink);
      }
    }
    py::capsule so = owner_of(series), to = owner_of(ts), bo = owner_of(block);
    if (!series || !ts || !block) throw std::bad_alloc();
    return make_parse_tuple(
        py::array_t<int32_t>({(py::ssize_t)nrows}, {4}, series, so),
        py::array_t<int64_t>({(py::ssize_t)nrows}, {8}, ts, to),
        sink, nrows, F0, bo);
  }

  // Steady-state ingest in one GIL-released pass (gdb_ingest::fused_ingest):
  // parse, route through the sid LUTs, build the packed row block in `stage`
  // and the per-region WAL payloads. Returns
  //   (0, n, counts, mins, maxs, [payload | None per region])   routed
  //   (1, (series, ts, fields, new_tagsets))    general path, parse() tuple
  //   (2, bytes_needed)                         stage too small; not parsed
  py::tuple ingest_batch(
      py::bytes data, py::array_t<int32_t, py::array::c_style> sid_region,
      py::array_t<int32_t, py::array::c_style> sid_local,
      py::array_t<int64_t, py::array::c_style> fmap, size_t n_parser_fields,
      int n_regions, py::bytes hdr_suffix, bool durable, int64_t ts_scale,
      py::array_t<uint8_t, py::array::c_style> stage) {
    char* buf;
    Py_ssize_t len;
    if (PyBytes_AsStringAndSize(data.ptr(), &buf, &len) != 0)
      throw std::runtime_error("expected bytes");
    if (sid_region.ndim() != 1 || sid_local.ndim() != 1 || fmap.ndim() != 1 ||
        stage.ndim() != 1 || sid_local.shape(0) != sid_region.shape(0))
      throw std::runtime_error("ingest_batch: bad argument shapes");
    char* sp = reinterpret_cast<char*>(stage.mutable_data());
    if (reinterpret_cast<uintptr_t>(sp) % 8 != 0)
      throw std::runtime_error("ingest_batch: stage must be 8-byte aligned");
    const std::string suffix = hdr_suffix;
    const size_t F0 = core_.num_fields();
    auto* res = new gdb_ingest::FusedResult();
    py::capsule keep(res, [](void* q) {
      delete static_cast<gdb_ingest::FusedResult*>(q);
    });
    {
      py::gil_scoped_release rel;
      gdb_ingest::fused_ingest(
          core_, buf, (size_t)len, sid_region.data(), sid_local.data(),
          (size_t)sid_region.shape(0), fmap.data(), (int)fmap.shape(0),
          n_parser_fields, n_regions, suffix, durable, ts_scale, sp,
          (size_t)stage.shape(0), *res);
    }
    if (res->status == gdb_ingest::FUSED_GROW)
      return py::make_tuple(2, res->need_bytes);
    if (res->status == gdb_ingest::FUSED_SLOW) {
      // hand the parse result over as fresh arrays (the stage is reused)
      const size_t n = res->n;
      py::array_t<int32_t> series((py::ssize_t)n);
      py::array_t<int64_t> ts((py::ssize_t)n);
      if (n) {
        std::memcpy(series.mutable_data(), res->sink.series, 4 * n);
        std::memcpy(ts.mutable_data(), res->sink.ts, 8 * n);
      }
      double* block = static_cast<double*>(std::malloc(8 * n * F0 + 8));
      py::capsule bo = owner_of(block);
      if (!block) throw std::bad_alloc();
      for (size_t c = 0; c < F0 && n; c++)
        std::memcpy(block + c * n, res->sink.col[c], 8 * n);
      for (size_t c = 0; c < F0; c++) res->sink.col[c] = block + c * n;
      return py::make_tuple(1, make_parse_tuple(
          std::move(series), std::move(ts), res->sink, n, F0, bo));
    }
    py::array_t<int64_t> counts(n_regions), mins(n_regions), maxs(n_regions);
    py::list payloads;
    if (res->n) {
      std::memcpy(counts.mutable_data(), res->counts.data(), 8 * (size_t)n_regions);
      std::memcpy(mins.mutable_data(), res->mins.data(), 8 * (size_t)n_regions);
      std::memcpy(maxs.mutable_data(), res->maxs.data(), 8 * (size_t)n_regions);
      for (int r = 0; r < n_regions; r++) {
        const size_t lo = res->wal_off[r], hi = res->wal_off[r + 1];
        if (hi == lo) {
          payloads.append(py::none());
        } else {   // view into the result's WAL arena (kept alive by `keep`)
          payloads.append(py::array_t<uint8_t>(
              {(py::ssize_t)(hi - lo)}, {1},
              reinterpret_cast<const uint8_t*>(res->wal.data() + lo), keep));
        }
      }
    }
    return py::make_tuple(0, res->n, std::move(counts), std::move(mins),
                          std::move(maxs), std::move(payloads));
  }

  size_t num_series() const { return core_.num_series(); }
  std::vector<std::string> field_names() const { return core_.field_names(); }
  size_t num_fields() const { return core_.num_fields(); }
  size_t intern_capacity() const { return core_.intern_capacity(); }

  py::bytes tagset_str(int32_t sid) const {
    const std::string* s = core_.tagset_str(sid);
    if (!s) throw std::out_of_range("unknown series ref");
    return py::bytes(*s);
  }

  // Restore dictionary state (e.g. after WAL replay / reopen).
  void register_tagset(const std::string& s, int32_t id) { core_.register_tagset(s, id); }
  void register_field(const std::string& name) { core_.register_field(name); }

 private:
  // (series, ts, {field: f64[n]}, new tagsets). Fields known before the
  // batch are views of the [F0, stride] block that `block_owner` frees;
  // fields first seen in the batch were parsed into sink.extra.
  py::tuple make_parse_tuple(py::array_t<int32_t> series, py::array_t<int64_t> ts,
                             gdb_ingest::ParseSink& sink, size_t n, size_t F0,
                             py::capsule block_owner) {
    const auto& names = core_.field_names();
    py::dict fields;
    for (size_t c = 0; c < names.size(); c++) {
      if (c < F0 && c < sink.col.size()) {
        fields[py::str(names[c])] = py::array_t<double>(
            {(py::ssize_t)n}, {8}, sink.col[c], block_owner);
      } else {
        py::array_t<double> a((py::ssize_t)n);
        if (n) {
          if (c < sink.col.size()) {
            std::memcpy(a.mutable_data(), sink.col[c], 8 * n);
          } else {
            std::fill(a.mutable_data(), a.mutable_data() + n, std::nan(""));
          }
        }
        fields[py::str(names[c])] = std::move(a);
      }
    }
    py::list newts;
    for (auto& [id, s] : sink.new_tagsets)
      newts.append(py::make_tuple(id, py::bytes(s)));
    return py::make_tuple(std::move(series), std::move(ts), std::move(fields),
                          std::move(newts));
  }

  gdb_ingest::LineCore core_;
};


// ---------------------------------------------------------------- WalWriter
// pybind glue over gdb_wal::WalWriter (csrc/wal_core.h). The writer is
// internally synchronized, so every call below runs its native part without
// the GIL.

// A payload argument: bytes or any contiguous buffer (the fused ingest path
// hands over uint8 views of its payload arena). Acquire and release under
// the GIL.
struct PayloadView {
  const uint8_t* p = nullptr;
  size_t n = 0;
  Py_buffer view;
  bool have_view = false;
  py::object owner;   // keeps a bytes payload alive while the GIL is released

  PayloadView() = default;
  PayloadView(const PayloadView&) = delete;
  PayloadView& operator=(const PayloadView&) = delete;
  ~PayloadView() { if (have_view) PyBuffer_Release(&view); }

  void acquire(PyObject* o) {
    owner = py::reinterpret_borrow<py::object>(o);
    if (PyBytes_Check(o)) {
      char* b; Py_ssize_t len;
      if (PyBytes_AsStringAndSize(o, &b, &len) != 0)
        throw std::runtime_error("payload must be bytes");
      p = reinterpret_cast<const uint8_t*>(b);
      n = (size_t)len;
    } else {
      if (PyObject_GetBuffer(o, &view, PyBUF_SIMPLE) != 0)
        throw py::error_already_set();
      have_view = true;
      p = static_cast<const uint8_t*>(view.buf);
      n = (size_t)view.len;
    }
  }
};

// Buffer one entry (group commit happens in commit()). Checksum and copy
// run without the GIL.
static void wal_writer_append(gdb_wal::WalWriter& w, uint64_t region_id,
                              uint64_t seq, py::object payload) {
  PayloadView v;
  v.acquire(payload.ptr());
  py::gil_scoped_release rel;
  w.append(region_id, seq, v.p, v.n);
}

// Write one frame per entry straight through to its writer's segment:
// entry i is (writers[i], region_ids[i], seqs[i], payloads[i]); a writer may
// appear more than once. All buffer views are taken first, then the GIL is
// released once for the whole call: every checksum is computed before any
// writer's mutex is taken, and each frame is written with writev from the
// caller's buffer (after whatever the writer still had buffered). With
// `sync`, each writer is fdatasync'ed once, after its last frame. Returns
// the segment size of each entry's writer after its frame.
static py::list wal_append_commit(py::list writers,
                                  std::vector<uint64_t> region_ids,
                                  std::vector<uint64_t> seqs,
                                  py::list payloads, bool sync) {
  const size_t m = (size_t)py::len(writers);
  if (region_ids.size() != m || seqs.size() != m || (size_t)py::len(payloads) != m)
    throw std::runtime_error("wal_append_commit: argument lists differ in length");
  std::vector<gdb_wal::WalWriter*> w(m);
  std::vector<py::object> writer_refs(m);
  std::vector<PayloadView> views(m);
  for (size_t i = 0; i < m; i++) {
    writer_refs[i] = writers[i];
    w[i] = py::cast<gdb_wal::WalWriter*>(writer_refs[i]);
    if (w[i] == nullptr)
      throw std::runtime_error("wal_append_commit: writer is None");
    views[i].acquire(py::object(payloads[i]).ptr());
  }
  std::vector<uint64_t> sizes(m, 0);
  std::string error;
  {
    py::gil_scoped_release rel;
    try {
      std::vector<uint8_t> hdrs(m * gdb_wal::kFrameHeaderBytes);
      for (size_t i = 0; i < m; i++)
        gdb_wal::frame_header(hdrs.data() + i * gdb_wal::kFrameHeaderBytes,
                              region_ids[i], seqs[i], views[i].p, views[i].n);
      for (size_t i = 0; i < m; i++) {
        bool last_of_writer = true;
        for (size_t j = i + 1; j < m && last_of_writer; j++)
          last_of_writer = w[j] != w[i];
        sizes[i] = w[i]->append_commit(
            hdrs.data() + i * gdb_wal::kFrameHeaderBytes, views[i].p,
            views[i].n, sync && last_of_writer);
      }
    } catch (const std::exception& e) {
      error = e.what();
      if (error.empty()) error = "wal_append_commit failed";
    }
  }
  if (!error.empty()) throw std::runtime_error(error);
  py::list out;
  for (size_t i = 0; i < m; i++) out.append(py::int_(sizes[i]));
  return out;
}

// Read back one WAL segment: returns list of (region_id, seq, payload bytes).
// Stops at the first corrupt/truncated frame (torn tail after crash).
static py::list wal_read_segment(const std::string& path) {
  std::vector<uint8_t> data;
  std::vector<gdb_wal::FrameView> frames;
  {
    py::gil_scoped_release rel;
    data = gdb_wal::read_file(path);
    frames = gdb_wal::read_frames(data.data(), data.size());
  }
  py::list out;
  for (const auto& f : frames)
    out.append(py::make_tuple(
        f.region, f.seq,
        py::bytes(reinterpret_cast<const char*>(f.payload), f.plen)));
  return out;
}

// zlib-compatible CRC-32 of a bytes-like object. impl: "auto" (what the WAL
// uses), "table" (slice-by-8) or "clmul" (raises on a CPU without it).
static uint32_t py_crc32(py::object data, uint32_t init, const std::string& impl) {
  PayloadView v;
  v.acquire(data.ptr());
  if (impl == "auto") return gdb_wal::crc32_update(init, v.p, v.n);
  if (impl == "table") return gdb_wal::crc32_table(init, v.p, v.n);
  if (impl == "clmul") return gdb_wal::crc32_clmul(init, v.p, v.n);
  throw std::invalid_argument("crc32: impl must be auto, table or clmul");
}

// ---------------------------------------------------------------- snappy
// Snappy block-format decompressor (format: google/snappy format_description.txt).
// Used for Prometheus remote write request bodies.

static bool snappy_uncompress(const uint8_t* in, size_t n, std::vector<uint8_t>& out) {
  size_t ip = 0;
  // preamble: uncompressed length varint
  uint64_t ulen = 0;
  int shift = 0;
  while (ip < n) {
    uint8_t b = in[ip++];
    ulen |= (uint64_t)(b & 0x7F) << shift;
    if (!(b & 0x80)) break;
    shift += 7;
    if (shift > 35) return false;
  }
  out.clear();
  out.reserve(ulen);
  while (ip < n) {
    const uint8_t tag = in[ip++];
    const int type = tag & 3;
    if (type == 0) {  // literal
      size_t len = (tag >> 2) + 1;
      if (len > 60) {
        const int extra = (int)len - 60;
        if (ip + extra > n) return false;
        len = 0;
        for (int i = 0; i < extra; i++) len |= (size_t)in[ip + i] << (8 * i);
        len += 1;
        ip += extra;
      }
      if (ip + len > n) return false;
      out.insert(out.end(), in + ip, in + ip + len);
      ip += len;
    } else {
      size_t len, off;
      if (type == 1) {
        if (ip >= n) return false;
        len = ((tag >> 2) & 7) + 4;
        off = ((size_t)(tag >> 5) << 8) | in[ip++];
      } else if (type == 2) {
        if (ip + 2 > n) return false;
        len = (tag >> 2) + 1;
        off = in[ip] | ((size_t)in[ip + 1] << 8);
        ip += 2;
      } else {
        if (ip + 4 > n) return false;
        len = (tag >> 2) + 1;
        off = in[ip] | ((size_t)in[ip + 1] << 8) |
              ((size_t)in[ip + 2] << 16) | ((size_t)in[ip + 3] << 24);
        ip += 4;
      }
      if (off == 0 || off > out.size()) return false;
      size_t src = out.size() - off;
      for (size_t i = 0; i < len; i++) out.push_back(out[src + i]);  // may overlap
    }
  }
  return out.size() == ulen;
}

static py::bytes py_snappy_uncompress(py::bytes data) {
  char* buf; Py_ssize_t len;
  if (PyBytes_AsStringAndSize(data.ptr(), &buf, &len) != 0)
    throw std::runtime_error("expected bytes");
  std::vector<uint8_t> out;
  if (!snappy_uncompress(reinterpret_cast<const uint8_t*>(buf), len, out))
    throw std::runtime_error("snappy: corrupt input");
  return py::bytes(reinterpret_cast<const char*>(out.data()), out.size());
}

// ------------------------------------------------- prometheus remote write
// Minimal protobuf wire parser for prometheus.WriteRequest:
//   WriteRequest{ repeated TimeSeries timeseries = 1 }
//   TimeSeries{ repeated Label labels = 1; repeated Sample samples = 2 }
//   Label{ string name = 1; string value = 2 }
//   Sample{ double value = 1; int64 timestamp = 2 }
// Label sets are interned (prometheus senders emit sorted labels) to dense
// series refs like the influx LineParser.

struct PwSlice { const uint8_t* p; size_t n; };

static inline uint64_t pw_varint(const uint8_t*& p, const uint8_t* end) {
  uint64_t v = 0;
  int shift = 0;
  while (p < end) {
    uint8_t b = *p++;
    v |= (uint64_t)(b & 0x7F) << shift;
    if (!(b & 0x80)) return v;
    shift += 7;
  }
  return v;
}

class PromWriteParser {
 public:
  // Returns (series i32[n], ts i64[n] ms, value f64[n],
  //          new_series [(id, metric, [(name,value)...])])
  py::tuple parse(py::bytes compressed, bool is_snappy) {
    char* buf; Py_ssize_t len;
    if (PyBytes_AsStringAndSize(compressed.ptr(), &buf, &len) != 0)
      throw std::runtime_error("expected bytes");
    std::vector<uint8_t> plain;
    const uint8_t* data;
    size_t n;
    if (is_snappy) {
      if (!snappy_uncompress(reinterpret_cast<const uint8_t*>(buf), len, plain))
        throw std::runtime_error("snappy: corrupt input");
      data = plain.data(); n = plain.size();
    } else {
      data = reinterpret_cast<const uint8_t*>(buf); n = len;
    }
    std::vector<int32_t> series;
    std::vector<int64_t> ts;
    std::vector<double> vals;
    py::list new_series;
    {
      const uint8_t* p = data;
      const uint8_t* end = data + n;
      while (p < end) {
        uint64_t key = pw_varint(p, end);
        if ((key >> 3) == 1 && (key & 7) == 2) {
          uint64_t tlen = pw_varint(p, end);
          parse_timeseries(p, p + tlen, series, ts, vals, new_series);
          p += tlen;
        } else {
          skip_field(key & 7, p, end);
        }
      }
    }
    py::array_t<int32_t> s(series.size());
    py::array_t<int64_t> t(ts.size());
    py::array_t<double> v(vals.size());
    std::memcpy(s.mutable_data(), series.data(), series.size() * 4);
    std::memcpy(t.mutable_data(), ts.data(), ts.size() * 8);
    std::memcpy(v.mutable_data(), vals.data(), vals.size() * 8);
    return py::make_tuple(std::move(s), std::move(t), std::move(v), std::move(new_series));
  }

  size_t num_series() const { return next_id_; }

 private:
  static void skip_field(int wt, const uint8_t*& p, const uint8_t* end) {
    if (wt == 0) { pw_varint(p, end); }
    else if (wt == 1) { p += 8; }
    else if (wt == 2) { uint64_t l = pw_varint(p, end); p += l; }
    else if (wt == 5) { p += 4; }
    else { p = end; }
  }

  void parse_timeseries(const uint8_t* p, const uint8_t* end,
                        std::vector<int32_t>& series, std::vector<int64_t>& ts,
                        std::vector<double>& vals, py::list& new_series) {
    // first pass: find label region bounds to build the intern key
    const uint8_t* q = p;
    std::string key;  // concatenated raw Label messages — canonical per sender
    std::vector<std::pair<std::string, std::string>> labels;
    std::vector<std::pair<double, int64_t>> samples;
    while (q < end) {
      uint64_t k = pw_varint(q, end);
      const int fnum = (int)(k >> 3), wt = (int)(k & 7);
      if (fnum == 1 && wt == 2) {          // Label
        uint64_t l = pw_varint(q, end);
        key.append(reinterpret_cast<const char*>(q), l);
        key.push_back('\xff');
        const uint8_t* lp = q;
        const uint8_t* lend = q + l;
        std::string lname, lval;
        while (lp < lend) {
          uint64_t lk = pw_varint(lp, lend);
          if ((lk >> 3) == 1 && (lk & 7) == 2) {
            uint64_t s = pw_varint(lp, lend);
            lname.assign(reinterpret_cast<const char*>(lp), s);
            lp += s;
          } else if ((lk >> 3) == 2 && (lk & 7) == 2) {
            uint64_t s = pw_varint(lp, lend);
            lval.assign(reinterpret_cast<const char*>(lp), s);
            lp += s;
          } else {
            skip_field(lk & 7, lp, lend);
          }
        }
        labels.emplace_back(std::move(lname), std::move(lval));
        q += l;
      } else if (fnum == 2 && wt == 2) {   // Sample
        uint64_t l = pw_varint(q, end);
        const uint8_t* sp = q;
        const uint8_t* send = q + l;
        double v = std::nan("");
        int64_t t = 0;
        while (sp < send) {
          uint64_t sk = pw_varint(sp, send);
          if ((sk >> 3) == 1 && (sk & 7) == 1) {
            std::memcpy(&v, sp, 8); sp += 8;
          } else if ((sk >> 3) == 2 && (sk & 7) == 0) {
            t = (int64_t)pw_varint(sp, send);
          } else {
            skip_field(sk & 7, sp, send);
          }
        }
        samples.emplace_back(v, t);
        q += l;
      } else {
        skip_field(wt, q, end);
      }
    }
    if (samples.empty()) return;
    const uint64_t h = fnv1a(key.data(), key.size());
    int32_t sid = -1;
    auto range = ids_.equal_range(h);
    for (auto it = range.first; it != range.second; ++it) {
      if (keys_[it->second] == key) { sid = it->second; break; }
    }
    if (sid < 0) {
      sid = next_id_++;
      ids_.emplace(h, sid);
      keys_.resize(std::max<size_t>(keys_.size(), sid + 1));
      keys_[sid] = key;
      std::string metric;
      py::list ls;
      for (auto& [ln, lv] : labels) {
        if (ln == "__name__") metric = lv;
        else ls.append(py::make_tuple(ln, lv));
      }
      new_series.append(py::make_tuple(sid, metric, std::move(ls)));
    }
    for (auto& [v, t] : samples) {
      series.push_back(sid);
      ts.push_back(t);
      vals.push_back(v);
    }
  }

  std::unordered_multimap<uint64_t, int32_t> ids_;
  std::vector<std::string> keys_;
  int32_t next_id_ = 0;
};

// ------------------------------------------------- OTLP traces (protobuf)
// Minimal wire parser for opentelemetry ExportTraceServiceRequest
// (trace.proto): resource_spans → scope_spans → spans. (service.name,
// span name) pairs are interned to dense series refs; ids come back as hex
// strings; attributes flatten to a compact JSON string column.

static const char* HEXD = "0123456789abcdef";

static std::string to_hex(const uint8_t* p, size_t n) {
  std::string s(n * 2, '0');
  for (size_t i = 0; i < n; i++) {
    s[2 * i] = HEXD[p[i] >> 4];
    s[2 * i + 1] = HEXD[p[i] & 0xF];
  }
  return s;
}

static void json_escape_into(std::string& out, const char* p, size_t n) {
  for (size_t i = 0; i < n; i++) {
    char c = p[i];
    if (c == '"' || c == '\\') { out.push_back('\\'); out.push_back(c); }
    else if ((unsigned char)c < 0x20) { out += "\\u0020"; }
    else out.push_back(c);
  }
}

class OtlpTraceParser {
 public:
  py::tuple parse(py::bytes data) {
    char* buf; Py_ssize_t len;
    if (PyBytes_AsStringAndSize(data.ptr(), &buf, &len) != 0)
      throw std::runtime_error("expected bytes");
    const uint8_t* p = reinterpret_cast<const uint8_t*>(buf);
    const uint8_t* end = p + len;
    out_series_.clear(); out_start_.clear(); out_dur_.clear();
    out_status_.clear();
    py::list trace_ids, span_ids, parent_ids, attrs, new_series;
    while (p < end) {
      uint64_t key = pw_varint(p, end);
      if ((key >> 3) == 1 && (key & 7) == 2) {
        uint64_t l = pw_varint(p, end);
        parse_resource_spans(p, p + l, trace_ids, span_ids, parent_ids,
                             attrs, new_series);
        p += l;
      } else {
        skip(key & 7, p, end);
      }
    }
    size_t n = out_series_.size();
    py::array_t<int32_t> s(n);
    py::array_t<int64_t> st(n);
    py::array_t<double> du(n);
    py::array_t<int32_t> stc(n);
    if (n) {
      std::memcpy(s.mutable_data(), out_series_.data(), n * 4);
      std::memcpy(st.mutable_data(), out_start_.data(), n * 8);
      std::memcpy(du.mutable_data(), out_dur_.data(), n * 8);
      std::memcpy(stc.mutable_data(), out_status_.data(), n * 4);
    }
    return py::make_tuple(std::move(s), std::move(st), std::move(du),
                          std::move(stc), std::move(trace_ids),
                          std::move(span_ids), std::move(parent_ids),
                          std::move(attrs), std::move(new_series));
  }

  size_t num_series() const { return next_id_; }

 private:
  static void skip(int wt, const uint8_t*& p, const uint8_t* end) {
    if (wt == 0) pw_varint(p, end);
    else if (wt == 1) p += 8;
    else if (wt == 2) { uint64_t l = pw_varint(p, end); p += l; }
    else if (wt == 5) p += 4;
    else p = end;
  }

  // returns value of attribute "service.name" from a Resource message
  std::string parse_resource_service(const uint8_t* p, const uint8_t* end) {
    std::string service = "unknown";
    while (p < end) {
      uint64_t k = pw_varint(p, end);
      if ((k >> 3) == 1 && (k & 7) == 2) {  // attributes: KeyValue
        uint64_t l = pw_varint(p, end);
        const uint8_t* kp = p; const uint8_t* kend = p + l;
        std::string kname, vstr;
        while (kp < kend) {
          uint64_t kk = pw_varint(kp, kend);
          if ((kk >> 3) == 1 && (kk & 7) == 2) {
            uint64_t s = pw_varint(kp, kend);
            kname.assign(reinterpret_cast<const char*>(kp), s); kp += s;
          } else if ((kk >> 3) == 2 && (kk & 7) == 2) {  // AnyValue
            uint64_t s = pw_varint(kp, kend);
            const uint8_t* vp = kp; const uint8_t* vend = kp + s;
            while (vp < vend) {
              uint64_t vk = pw_varint(vp, vend);
              if ((vk >> 3) == 1 && (vk & 7) == 2) {
                uint64_t sl = pw_varint(vp, vend);
                vstr.assign(reinterpret_cast<const char*>(vp), sl); vp += sl;
              } else skip(vk & 7, vp, vend);
            }
            kp += s;
          } else skip(kk & 7, kp, kend);
        }
        if (kname == "service.name" && !vstr.empty()) service = vstr;
        p += l;
      } else skip(k & 7, p, end);
    }
    return service;
  }

  void parse_resource_spans(const uint8_t* p, const uint8_t* end,
                            py::list& tids, py::list& sids, py::list& pids,
                            py::list& attrs, py::list& new_series) {
    std::string service = "unknown";
    while (p < end) {
      uint64_t k = pw_varint(p, end);
      int f = (int)(k >> 3), wt = (int)(k & 7);
      if (f == 1 && wt == 2) {  // Resource
        uint64_t l = pw_varint(p, end);
        service = parse_resource_service(p, p + l);
        p += l;
      } else if (f == 2 && wt == 2) {  // ScopeSpans
        uint64_t l = pw_varint(p, end);
        const uint8_t* sp = p; const uint8_t* send = p + l;
        while (sp < send) {
          uint64_t sk = pw_varint(sp, send);
          if ((sk >> 3) == 2 && (sk & 7) == 2) {  // Span
            uint64_t sl = pw_varint(sp, send);
            parse_span(sp, sp + sl, service, tids, sids, pids, attrs, new_series);
            sp += sl;
          } else skip(sk & 7, sp, send);
        }
        p += l;
      } else skip(wt, p, end);
    }
  }

  void parse_span(const uint8_t* p, const uint8_t* end, const std::string& service,
                  py::list& tids, py::list& sids, py::list& pids,
                  py::list& attrs, py::list& new_series) {
    std::string trace_id, span_id, parent_id, name;
    uint64_t start = 0, stop = 0;
    int32_t status = 0;
    std::string attr_json = "{";
    bool first_attr = true;
    while (p < end) {
      uint64_t k = pw_varint(p, end);
      int f = (int)(k >> 3), wt = (int)(k & 7);
      if (f == 1 && wt == 2) {
        uint64_t l = pw_varint(p, end);
        trace_id = to_hex(p, l); p += l;
      } else if (f == 2 && wt == 2) {
        uint64_t l = pw_varint(p, end);
        span_id = to_hex(p, l); p += l;
      } else if (f == 4 && wt == 2) {
        uint64_t l = pw_varint(p, end);
        parent_id = to_hex(p, l); p += l;
      } else if (f == 5 && wt == 2) {
        uint64_t l = pw_varint(p, end);
        name.assign(reinterpret_cast<const char*>(p), l); p += l;
      } else if (f == 7 && wt == 1) {
        std::memcpy(&start, p, 8); p += 8;
      } else if (f == 8 && wt == 1) {
        std::memcpy(&stop, p, 8); p += 8;
      } else if (f == 9 && wt == 2) {  // attributes KeyValue
        uint64_t l = pw_varint(p, end);
        append_attr_json(p, p + l, attr_json, first_attr);
        p += l;
      } else if (f == 15 && wt == 2) {  // Status{message=2?, code=3? -> code=2? }
        uint64_t l = pw_varint(p, end);
        const uint8_t* qp = p; const uint8_t* qend = p + l;
        while (qp < qend) {
          uint64_t qk = pw_varint(qp, qend);
          if ((qk >> 3) == 2 && (qk & 7) == 0) {
            status = (int32_t)pw_varint(qp, qend);
          } else if ((qk >> 3) == 3 && (qk & 7) == 0) {
            status = (int32_t)pw_varint(qp, qend);
          } else skip(qk & 7, qp, qend);
        }
        p += l;
      } else {
        skip(wt, p, end);
      }
    }
    attr_json.push_back('}');
    // intern (service, span name)
    std::string key = service;
    key.push_back('\0');
    key += name;
    const uint64_t h = fnv1a(key.data(), key.size());
    int32_t sid = -1;
    auto range = ids_.equal_range(h);
    for (auto it = range.first; it != range.second; ++it)
      if (keys_[it->second] == key) { sid = it->second; break; }
    if (sid < 0) {
      sid = next_id_++;
      ids_.emplace(h, sid);
      keys_.resize(std::max<size_t>(keys_.size(), sid + 1));
      keys_[sid] = key;
      new_series.append(py::make_tuple(sid, py::str(service), py::str(name)));
    }
    out_series_.push_back(sid);
    out_start_.push_back((int64_t)start);
    out_dur_.push_back(stop >= start ? (double)(stop - start) / 1e6 : 0.0);  // ms
    out_status_.push_back(status);
    tids.append(py::str(trace_id));
    sids.append(py::str(span_id));
    pids.append(py::str(parent_id));
    attrs.append(py::str(attr_json));
  }

  void append_attr_json(const uint8_t* p, const uint8_t* end, std::string& out,
                        bool& first) {
    std::string kname, vjson;
    while (p < end) {
      uint64_t k = pw_varint(p, end);
      if ((k >> 3) == 1 && (k & 7) == 2) {
        uint64_t l = pw_varint(p, end);
        kname.assign(reinterpret_cast<const char*>(p), l); p += l;
      } else if ((k >> 3) == 2 && (k & 7) == 2) {  // AnyValue
        uint64_t l = pw_varint(p, end);
        const uint8_t* vp = p; const uint8_t* vend = p + l;
        while (vp < vend) {
          uint64_t vk = pw_varint(vp, vend);
          int vf = (int)(vk >> 3), vwt = (int)(vk & 7);
          if (vf == 1 && vwt == 2) {
            uint64_t sl = pw_varint(vp, vend);
            vjson = "\"";
            json_escape_into(vjson, reinterpret_cast<const char*>(vp), sl);
            vjson += "\"";
            vp += sl;
          } else if (vf == 2 && vwt == 0) {
            vjson = pw_varint(vp, vend) ? "true" : "false";
          } else if (vf == 3 && vwt == 0) {
            vjson = std::to_string((int64_t)pw_varint(vp, vend));
          } else if (vf == 4 && vwt == 1) {
            double d; std::memcpy(&d, vp, 8); vp += 8;
            vjson = std::to_string(d);
          } else skip(vwt, vp, vend);
        }
        p += l;
      } else skip(k & 7, p, end);
    }
    if (!kname.empty() && !vjson.empty()) {
      if (!first) out.push_back(',');
      first = false;
      out.push_back('"');
      json_escape_into(out, kname.data(), kname.size());
      out += "\":";
      out += vjson;
    }
  }

  std::unordered_multimap<uint64_t, int32_t> ids_;
  std::vector<std::string> keys_;
  int32_t next_id_ = 0;
  std::vector<int32_t> out_series_;
  std::vector<int64_t> out_start_;
  std::vector<double> out_dur_;
  std::vector<int32_t> out_status_;
};

// ------------------------------------------------- OTLP metrics + logs
// ExportMetricsServiceRequest: resource_metrics → scope_metrics → Metric
// { name=1; gauge=5 / sum=7 { data_points: NumberDataPoint } }.
// NumberDataPoint{ attributes=7; time_unix_nano=3 (fixed64);
//                  as_double=4 (fixed64) / as_int=6 (sfixed64) }.
// Output: flat [(metric, {attrs}, ts_ms, value)] ready for
// PromStore.write_points.

class OtlpMetricsParser {
 public:
  py::list parse(py::bytes data) {
    char* buf; Py_ssize_t len;
    if (PyBytes_AsStringAndSize(data.ptr(), &buf, &len) != 0)
      throw std::runtime_error("expected bytes");
    py::list out;
    const uint8_t* p = reinterpret_cast<const uint8_t*>(buf);
    const uint8_t* end = p + len;
    while (p < end) {
      uint64_t k = pw_varint(p, end);
      if ((k >> 3) == 1 && (k & 7) == 2) {
        uint64_t l = pw_varint(p, end);
        parse_resource_metrics(p, p + l, out);
        p += l;
      } else skip(k & 7, p, end);
    }
    return out;
  }

 private:
  static void skip(int wt, const uint8_t*& p, const uint8_t* end) {
    if (wt == 0) pw_varint(p, end);
    else if (wt == 1) p += 8;
    else if (wt == 2) { uint64_t l = pw_varint(p, end); p += l; }
    else if (wt == 5) p += 4;
    else p = end;
  }

  static void parse_kv(const uint8_t* p, const uint8_t* end, py::dict& attrs) {
    std::string kname, vstr;
    double vnum = 0; bool has_num = false;
    while (p < end) {
      uint64_t k = pw_varint(p, end);
      if ((k >> 3) == 1 && (k & 7) == 2) {
        uint64_t l = pw_varint(p, end);
        kname.assign(reinterpret_cast<const char*>(p), l); p += l;
      } else if ((k >> 3) == 2 && (k & 7) == 2) {
        uint64_t l = pw_varint(p, end);
        const uint8_t* vp = p; const uint8_t* vend = p + l;
        while (vp < vend) {
          uint64_t vk = pw_varint(vp, vend);
          int vf = (int)(vk >> 3), vwt = (int)(vk & 7);
          if (vf == 1 && vwt == 2) {
            uint64_t sl = pw_varint(vp, vend);
            vstr.assign(reinterpret_cast<const char*>(vp), sl); vp += sl;
          } else if (vf == 2 && vwt == 0) {
            vstr = pw_varint(vp, vend) ? "true" : "false";
          } else if (vf == 3 && vwt == 0) {
            vstr = std::to_string((int64_t)pw_varint(vp, vend));
          } else if (vf == 4 && vwt == 1) {
            double d; std::memcpy(&d, vp, 8); vp += 8;
            vstr = std::to_string(d);
          } else skip(vwt, vp, vend);
        }
        p += l;
      } else skip(k & 7, p, end);
    }
    if (!kname.empty()) attrs[py::str(kname)] = py::str(vstr);
  }

  void parse_resource_metrics(const uint8_t* p, const uint8_t* end, py::list& out) {
    py::dict res_attrs;
    while (p < end) {
      uint64_t k = pw_varint(p, end);
      int f = (int)(k >> 3), wt = (int)(k & 7);
      if (f == 1 && wt == 2) {  // Resource{attributes=1}
        uint64_t l = pw_varint(p, end);
        const uint8_t* rp = p; const uint8_t* rend = p + l;
        while (rp < rend) {
          uint64_t rk = pw_varint(rp, rend);
          if ((rk >> 3) == 1 && (rk & 7) == 2) {
            uint64_t al = pw_varint(rp, rend);
            parse_kv(rp, rp + al, res_attrs);
            rp += al;
          } else skip(rk & 7, rp, rend);
        }
        p += l;
      } else if (f == 2 && wt == 2) {  // ScopeMetrics
        uint64_t l = pw_varint(p, end);
        const uint8_t* sp = p; const uint8_t* send = p + l;
        while (sp < send) {
          uint64_t sk = pw_varint(sp, send);
          if ((sk >> 3) == 2 && (sk & 7) == 2) {  // Metric
            uint64_t ml = pw_varint(sp, send);
            parse_metric(sp, sp + ml, res_attrs, out);
            sp += ml;
          } else skip(sk & 7, sp, send);
        }
        p += l;
      } else skip(wt, p, end);
    }
  }

  void parse_metric(const uint8_t* p, const uint8_t* end,
                    const py::dict& res_attrs, py::list& out) {
    std::string name;
    while (p < end) {
      uint64_t k = pw_varint(p, end);
      int f = (int)(k >> 3), wt = (int)(k & 7);
      if (f == 1 && wt == 2) {
        uint64_t l = pw_varint(p, end);
        name.assign(reinterpret_cast<const char*>(p), l); p += l;
      } else if ((f == 5 || f == 7) && wt == 2) {  // Gauge / Sum
        uint64_t l = pw_varint(p, end);
        const uint8_t* gp = p; const uint8_t* gend = p + l;
        while (gp < gend) {
          uint64_t gk = pw_varint(gp, gend);
          if ((gk >> 3) == 1 && (gk & 7) == 2) {   // data_points
            uint64_t dl = pw_varint(gp, gend);
            parse_point(gp, gp + dl, name, res_attrs, out);
            gp += dl;
          } else skip(gk & 7, gp, gend);
        }
        p += l;
      } else skip(wt, p, end);
    }
  }

  void parse_point(const uint8_t* p, const uint8_t* end, const std::string& name,
                   const py::dict& res_attrs, py::list& out) {
    py::dict attrs;
    for (auto item : res_attrs) attrs[item.first] = item.second;
    uint64_t ts = 0;
    double val = 0;
    while (p < end) {
      uint64_t k = pw_varint(p, end);
      int f = (int)(k >> 3), wt = (int)(k & 7);
      if (f == 7 && wt == 2) {
        uint64_t l = pw_varint(p, end);
        parse_kv(p, p + l, attrs);
        p += l;
      } else if (f == 3 && wt == 1) {
        std::memcpy(&ts, p, 8); p += 8;
      } else if (f == 4 && wt == 1) {
        std::memcpy(&val, p, 8); p += 8;
      } else if (f == 6 && wt == 1) {
        int64_t iv; std::memcpy(&iv, p, 8); p += 8;
        val = (double)iv;
      } else skip(wt, p, end);
    }
    out.append(py::make_tuple(py::str(name), std::move(attrs),
                              (int64_t)(ts / 1000000ULL), val));
  }
};

// ExportLogsServiceRequest: resource_logs → scope_logs → LogRecord
// { time_unix_nano=1 fixed64; severity_text=3; body=5 AnyValue;
//   attributes=6 }. Output: [(ts_ms, severity, body, {attrs})].
class OtlpLogsParser {
 public:
  py::list parse(py::bytes data) {
    char* buf; Py_ssize_t len;
    if (PyBytes_AsStringAndSize(data.ptr(), &buf, &len) != 0)
      throw std::runtime_error("expected bytes");
    py::list out;
    const uint8_t* p = reinterpret_cast<const uint8_t*>(buf);
    const uint8_t* end = p + len;
    while (p < end) {
      uint64_t k = pw_varint(p, end);
      if ((k >> 3) == 1 && (k & 7) == 2) {
        uint64_t l = pw_varint(p, end);
        const uint8_t* rp = p; const uint8_t* rend = p + l;
        std::string service = "unknown";
        while (rp < rend) {
          uint64_t rk = pw_varint(rp, rend);
          int f = (int)(rk >> 3), wt = (int)(rk & 7);
          if (f == 1 && wt == 2) {  // Resource (attrs ignored; senders put
            uint64_t rl = pw_varint(rp, rend);   // routing labels on records)
            rp += rl;
          } else if (f == 2 && wt == 2) {  // ScopeLogs
            uint64_t sl = pw_varint(rp, rend);
            const uint8_t* lp = rp; const uint8_t* lend = rp + sl;
            while (lp < lend) {
              uint64_t lk = pw_varint(lp, lend);
              if ((lk >> 3) == 2 && (lk & 7) == 2) {  // LogRecord
                uint64_t ll = pw_varint(lp, lend);
                parse_record(lp, lp + ll, out);
                lp += ll;
              } else OtlpMetricsSkip(lk & 7, lp, lend);
            }
            rp += sl;
          } else OtlpMetricsSkip(wt, rp, rend);
        }
        p += l;
      } else OtlpMetricsSkip(k & 7, p, end);
    }
    return out;
  }

 private:
  static void OtlpMetricsSkip(int wt, const uint8_t*& p, const uint8_t* end) {
    if (wt == 0) pw_varint(p, end);
    else if (wt == 1) p += 8;
    else if (wt == 2) { uint64_t l = pw_varint(p, end); p += l; }
    else if (wt == 5) p += 4;
    else p = end;
  }

  void parse_record(const uint8_t* p, const uint8_t* end, py::list& out) {
    uint64_t ts = 0;
    std::string severity, body;
    py::dict attrs;
    while (p < end) {
      uint64_t k = pw_varint(p, end);
      int f = (int)(k >> 3), wt = (int)(k & 7);
      if (f == 1 && wt == 1) {
        std::memcpy(&ts, p, 8); p += 8;
      } else if (f == 3 && wt == 2) {
        uint64_t l = pw_varint(p, end);
        severity.assign(reinterpret_cast<const char*>(p), l); p += l;
      } else if (f == 5 && wt == 2) {  // body AnyValue{string_value=1}
        uint64_t l = pw_varint(p, end);
        const uint8_t* bp = p; const uint8_t* bend = p + l;
        while (bp < bend) {
          uint64_t bk = pw_varint(bp, bend);
          if ((bk >> 3) == 1 && (bk & 7) == 2) {
            uint64_t sl = pw_varint(bp, bend);
            body.assign(reinterpret_cast<const char*>(bp), sl); bp += sl;
          } else OtlpMetricsSkip(bk & 7, bp, bend);
        }
        p += l;
      } else if (f == 6 && wt == 2) {
        uint64_t l = pw_varint(p, end);
        // KeyValue (string values only, like metrics attrs)
        const uint8_t* kp = p; const uint8_t* kend = p + l;
        std::string kname, vstr;
        while (kp < kend) {
          uint64_t kk = pw_varint(kp, kend);
          if ((kk >> 3) == 1 && (kk & 7) == 2) {
            uint64_t s = pw_varint(kp, kend);
            kname.assign(reinterpret_cast<const char*>(kp), s); kp += s;
          } else if ((kk >> 3) == 2 && (kk & 7) == 2) {
            uint64_t s = pw_varint(kp, kend);
            const uint8_t* vp = kp; const uint8_t* vend = kp + s;
            while (vp < vend) {
              uint64_t vk = pw_varint(vp, vend);
              if ((vk >> 3) == 1 && (vk & 7) == 2) {
                uint64_t sl = pw_varint(vp, vend);
                vstr.assign(reinterpret_cast<const char*>(vp), sl); vp += sl;
              } else OtlpMetricsSkip(vk & 7, vp, vend);
            }
            kp += s;
          } else OtlpMetricsSkip(kk & 7, kp, kend);
        }
        if (!kname.empty()) attrs[py::str(kname)] = py::str(vstr);
        p += l;
      } else OtlpMetricsSkip(wt, p, end);
    }
    out.append(py::make_tuple((int64_t)(ts / 1000000ULL), py::str(severity),
                              py::str(body), std::move(attrs)));
  }
};

// ---------------------------------------------------------------- tokenizer
// Fulltext tokenizer for log columns (reference: src/index fulltext_index —
// tantivy's default tokenizer ≈ lowercase alphanumeric runs). Terms are
// interned region-wide; output is CSR (doc offsets + term ids) ready to
// build GPU posting lists.

class Tokenizer {
 public:
  // docs: list[str|bytes]. Returns (offsets u64[n+1], term_ids i32[total],
  // new_terms [(id, str)...]).
  py::tuple tokenize(py::list docs) {
    std::vector<uint64_t> offsets;
    std::vector<int32_t> ids;
    py::list new_terms;
    offsets.reserve(docs.size() + 1);
    offsets.push_back(0);
    std::vector<int32_t> doc_terms;
    for (auto& d : docs) {
      char* buf = nullptr;
      Py_ssize_t blen = 0;
      std::string tmp;
      if (PyBytes_Check(d.ptr())) {
        PyBytes_AsStringAndSize(d.ptr(), &buf, &blen);
      } else if (PyUnicode_Check(d.ptr())) {
        tmp = py::cast<std::string>(d);
        buf = tmp.data();
        blen = tmp.size();
      }
      doc_terms.clear();
      size_t i = 0;
      while (i < (size_t)blen) {
        while (i < (size_t)blen && !isalnum((unsigned char)buf[i])) i++;
        size_t s = i;
        while (i < (size_t)blen && isalnum((unsigned char)buf[i])) i++;
        if (i > s) {
          std::string term(buf + s, i - s);
          for (auto& c : term) c = tolower((unsigned char)c);
          const uint64_t h = fnv1a(term.data(), term.size());
          int32_t tid = -1;
          auto range = tmap_.equal_range(h);
          for (auto it = range.first; it != range.second; ++it)
            if (terms_[it->second] == term) { tid = it->second; break; }
          if (tid < 0) {
            tid = (int32_t)terms_.size();
            tmap_.emplace(h, tid);
            terms_.push_back(term);
            new_terms.append(py::make_tuple(tid, py::str(term)));
          }
          // dedupe within doc (posting lists store docs, not positions)
          bool seen = false;
          for (int32_t t : doc_terms) if (t == tid) { seen = true; break; }
          if (!seen) doc_terms.push_back(tid);
        }
      }
      ids.insert(ids.end(), doc_terms.begin(), doc_terms.end());
      offsets.push_back(ids.size());
    }
    py::array_t<uint64_t> off(offsets.size());
    py::array_t<int32_t> tid(ids.size());
    std::memcpy(off.mutable_data(), offsets.data(), offsets.size() * 8);
    if (!ids.empty()) std::memcpy(tid.mutable_data(), ids.data(), ids.size() * 4);
    return py::make_tuple(std::move(off), std::move(tid), std::move(new_terms));
  }

  // term → id (-1 if unknown); query-side probe
  int32_t term_id(const std::string& term_in) const {
    std::string term = term_in;
    for (auto& c : term) c = tolower((unsigned char)c);
    const uint64_t h = fnv1a(term.data(), term.size());
    auto range = tmap_.equal_range(h);
    for (auto it = range.first; it != range.second; ++it)
      if (terms_[it->second] == term) return it->second;
    return -1;
  }

  size_t num_terms() const { return terms_.size(); }

  // get-or-create id for an already-normalized term (persisted fulltext
  // sidecar load: terms come back verbatim from the index file, no doc
  // re-tokenization)
  int32_t intern(const std::string& term) {
    const uint64_t h = fnv1a(term.data(), term.size());
    auto range = tmap_.equal_range(h);
    for (auto it = range.first; it != range.second; ++it)
      if (terms_[it->second] == term) return it->second;
    int32_t tid = (int32_t)terms_.size();
    tmap_.emplace(h, tid);
    terms_.push_back(term);
    return tid;
  }

  // bulk variant: lens i32[k] + concatenated utf8 blob → ids i32[k]
  py::array_t<int32_t> intern_blob(py::array_t<int32_t> lens, py::bytes blob) {
    char* buf = nullptr;
    Py_ssize_t blen = 0;
    PyBytes_AsStringAndSize(blob.ptr(), &buf, &blen);
    const int32_t* ln = lens.data();
    const size_t k = lens.size();
    py::array_t<int32_t> out(k);
    int32_t* o = out.mutable_data();
    size_t off = 0;
    for (size_t i = 0; i < k; i++) {
      o[i] = intern(std::string(buf + off, ln[i]));
      off += ln[i];
    }
    return out;
  }

  py::str term_str(int32_t tid) const {
    if (tid < 0 || (size_t)tid >= terms_.size())
      throw std::out_of_range("tid");
    return py::str(terms_[tid]);
  }

 private:
  std::unordered_multimap<uint64_t, int32_t> tmap_;
  std::vector<std::string> terms_;
};

// Pack a python string column (list of str|None) into (lens i32, utf8 blob)
// — WAL string-field serialization hot path.
static py::tuple pack_str_col(py::list vals) {
  const size_t n = vals.size();
  py::array_t<int32_t> lens(n);
  int32_t* lp = lens.mutable_data();
  std::string blob;
  blob.reserve(n * 16);
  for (size_t i = 0; i < n; i++) {
    PyObject* o = vals[i].ptr();
    if (o == Py_None) {
      lp[i] = -1;
    } else if (PyUnicode_Check(o)) {
      Py_ssize_t sl;
      const char* s = PyUnicode_AsUTF8AndSize(o, &sl);
      lp[i] = (int32_t)sl;
      blob.append(s, sl);
    } else if (PyBytes_Check(o)) {
      char* s; Py_ssize_t sl;
      PyBytes_AsStringAndSize(o, &s, &sl);
      lp[i] = (int32_t)sl;
      blob.append(s, sl);
    } else {
      lp[i] = -1;
    }
  }
  return py::make_tuple(std::move(lens), py::bytes(blob));
}

// One-pass ingest router (K16 host side): per-region WAL payload bodies,
// destination offsets for the scatter_append kernel, and per-region
// counts/min/max — replaces the python argsort + per-region numpy fancy
// gathers on the ingest hot path. Payload layout matches wal.encode_batch:
// [u32 hdr_len][hdr json][i32 codes][i64 ts][f64 fields nf*m].
// `hdr_suffix` is the cached per-table json tail: everything after the
// numeric value of "n" (b', "fields": [...], "strs": [], ...}').
static py::tuple route_ingest(
    py::array_t<int32_t, py::array::c_style | py::array::forcecast> codes,
    py::array_t<int64_t, py::array::c_style | py::array::forcecast> ts,
    py::list field_arrs,          // parser field columns, each f64[n]
    py::array_t<int64_t, py::array::c_style | py::array::forcecast> fmap,
    py::array_t<int32_t, py::array::c_style | py::array::forcecast> region_of,
    int n_regions, py::bytes hdr_suffix, bool durable) {
  const int64_t n = codes.shape(0);
  const int nf = (int)fmap.shape(0);
  if (ts.shape(0) != n || region_of.shape(0) != n)
    throw std::runtime_error("route_ingest: length mismatch");
  const int32_t* cp = codes.data();
  const int64_t* tp = ts.data();
  const int64_t* fm = fmap.data();
  const int32_t* rp = region_of.data();
  std::string suffix = hdr_suffix;

  // assemble the table-ordered field matrix [nf, n] (fmap row -1 → NaN)
  std::vector<const double*> srcs(field_arrs.size());
  for (size_t i = 0; i < field_arrs.size(); i++) {
    auto a = py::cast<py::array_t<double,
        py::array::c_style | py::array::forcecast>>(field_arrs[i]);
    if (a.shape(0) != n) throw std::runtime_error("field length mismatch");
    srcs[i] = a.data();
    field_arrs[i] = a;   // keep the (possibly converted) arrays alive
  }
  py::array_t<double> out_mat({(py::ssize_t)nf, (py::ssize_t)n});
  double* fp = out_mat.mutable_data();
  {
    py::gil_scoped_release nogil;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int f = 0; f < nf; f++) {
      const int64_t s = fm[f];
      if (s < 0 || (size_t)s >= srcs.size()) {
        std::fill(fp + (int64_t)f * n, fp + (int64_t)(f + 1) * n, nan);
      } else {
        std::memcpy(fp + (int64_t)f * n, srcs[s], 8 * n);
      }
    }
  }

  py::array_t<int64_t> dst_off(n);
  py::array_t<int64_t> counts(n_regions), mins(n_regions), maxs(n_regions);
  int64_t* dp = dst_off.mutable_data();
  int64_t* cnt = counts.mutable_data();
  int64_t* mn = mins.mutable_data();
  int64_t* mx = maxs.mutable_data();
  for (int r = 0; r < n_regions; r++) {
    cnt[r] = 0;
    mn[r] = INT64_MAX;
    mx[r] = INT64_MIN;
  }
  {
    py::gil_scoped_release nogil;
    for (int64_t i = 0; i < n; i++) {
      const int32_t r = rp[i];
      dp[i] = cnt[r]++;
      const int64_t t = tp[i];
      if (t < mn[r]) mn[r] = t;
      if (t > mx[r]) mx[r] = t;
    }
  }

  py::list payloads;
  if (!durable) {
    for (int r = 0; r < n_regions; r++) payloads.append(py::none());
    return py::make_tuple(payloads, std::move(out_mat), std::move(dst_off),
                          std::move(counts), std::move(mins), std::move(maxs));
  }
  // allocate per-region payload buffers (header + columns)
  std::vector<char*> bufs(n_regions, nullptr);
  std::vector<int64_t> code_off(n_regions), ts_off(n_regions), f_off(n_regions);
  for (int r = 0; r < n_regions; r++) {
    if (cnt[r] == 0) {
      payloads.append(py::none());
      continue;
    }
    std::string hdr = "{\"n\": " + std::to_string(cnt[r]) + suffix;
    const int64_t m = cnt[r];
    const int64_t total = 4 + (int64_t)hdr.size() + 4 * m + 8 * m + 8LL * nf * m;
    PyObject* b = PyBytes_FromStringAndSize(nullptr, total);
    char* p = PyBytes_AS_STRING(b);
    const uint32_t hl = (uint32_t)hdr.size();
    std::memcpy(p, &hl, 4);
    std::memcpy(p + 4, hdr.data(), hl);
    bufs[r] = p;
    code_off[r] = 4 + hl;
    ts_off[r] = code_off[r] + 4 * m;
    f_off[r] = ts_off[r] + 8 * m;
    payloads.append(py::reinterpret_steal<py::object>(b));
  }
  {
    py::gil_scoped_release nogil;
    for (int64_t i = 0; i < n; i++) {
      const int32_t r = rp[i];
      char* p = bufs[r];
      const int64_t o = dp[i];
      const int64_t m = cnt[r];
      std::memcpy(p + code_off[r] + 4 * o, cp + i, 4);
      std::memcpy(p + ts_off[r] + 8 * o, tp + i, 8);
      char* fdst = p + f_off[r];
      for (int f = 0; f < nf; f++) {
        std::memcpy(fdst + 8 * ((int64_t)f * m + o), fp + (int64_t)f * n + i, 8);
      }
    }
  }
  return py::make_tuple(payloads, std::move(out_mat), std::move(dst_off),
                        std::move(counts), std::move(mins), std::move(maxs));
}

void register_pagedec(py::module_& m);

PYBIND11_MODULE(_native, m) {
  register_pagedec(m);
  m.doc() = "greptimedb_amd host-native ingest path (line parser + WAL)";
  py::class_<LineParser>(m, "LineParser")
      .def(py::init<>())
      .def("parse", &LineParser::parse)
      .def("ingest_batch", &LineParser::ingest_batch, py::arg("data"),
           py::arg("sid_region"), py::arg("sid_local"), py::arg("fmap"),
           py::arg("n_parser_fields"), py::arg("n_regions"),
           py::arg("hdr_suffix"), py::arg("durable"), py::arg("ts_scale"),
           py::arg("stage"))
      .def("num_fields", &LineParser::num_fields)
      .def("intern_capacity", &LineParser::intern_capacity)
      .def("num_series", &LineParser::num_series)
      .def("tagset_str", &LineParser::tagset_str)
      .def("field_names", &LineParser::field_names)
      .def("register_tagset", &LineParser::register_tagset)
      .def("register_field", &LineParser::register_field);
  py::class_<gdb_wal::WalWriter>(m, "WalWriter")
      .def(py::init<>())
      .def("open_segment", &gdb_wal::WalWriter::open_segment,
           py::call_guard<py::gil_scoped_release>())
      .def("close_segment", &gdb_wal::WalWriter::close_segment,
           py::arg("sync") = false, py::call_guard<py::gil_scoped_release>())
      .def("rotate", &gdb_wal::WalWriter::rotate, py::arg("path"),
           py::arg("sync") = false, py::call_guard<py::gil_scoped_release>())
      .def("append", &wal_writer_append)
      .def("commit", &gdb_wal::WalWriter::commit, py::arg("sync") = true,
           py::call_guard<py::gil_scoped_release>())
      // the accessors take the writer's mutex, which a write or sync in
      // another thread may hold for a while: wait for it without the GIL
      .def("segment_bytes", &gdb_wal::WalWriter::segment_bytes,
           py::call_guard<py::gil_scoped_release>())
      .def("unsynced_bytes", &gdb_wal::WalWriter::unsynced_bytes,
           py::call_guard<py::gil_scoped_release>())
      .def("sync_count", &gdb_wal::WalWriter::sync_count,
           py::call_guard<py::gil_scoped_release>());
  m.def("wal_append_commit", &wal_append_commit, py::arg("writers"),
        py::arg("region_ids"), py::arg("seqs"), py::arg("payloads"),
        py::arg("sync") = false);
  m.def("crc32", &py_crc32, py::arg("data"), py::arg("init") = 0,
        py::arg("impl") = "auto");
  m.def("crc32_have_clmul", &gdb_wal::crc32_have_clmul);
  m.def("crc32_force_table", [](bool on) {
    gdb_wal::crc32_force_table_flag().store(on);
  }, "measurement switch: make the \"auto\" CRC path use the table");
  m.def("wal_read_segment", &wal_read_segment);
  m.def("snappy_uncompress", &py_snappy_uncompress);
  m.def("pack_str_col", &pack_str_col);
  m.def("route_ingest", &route_ingest, "K16 host-side ingest router");
  py::class_<PromWriteParser>(m, "PromWriteParser")
      .def(py::init<>())
      .def("parse", &PromWriteParser::parse, py::arg("data"), py::arg("is_snappy") = true)
      .def("num_series", &PromWriteParser::num_series);
  py::class_<OtlpMetricsParser>(m, "OtlpMetricsParser")
      .def(py::init<>())
      .def("parse", &OtlpMetricsParser::parse);
  py::class_<OtlpLogsParser>(m, "OtlpLogsParser")
      .def(py::init<>())
      .def("parse", &OtlpLogsParser::parse);
  py::class_<OtlpTraceParser>(m, "OtlpTraceParser")
      .def(py::init<>())
      .def("parse", &OtlpTraceParser::parse)
      .def("num_series", &OtlpTraceParser::num_series);
  py::class_<Tokenizer>(m, "Tokenizer")
      .def(py::init<>())
      .def("tokenize", &Tokenizer::tokenize)
      .def("term_id", &Tokenizer::term_id)
      .def("intern", &Tokenizer::intern)
      .def("intern_blob", &Tokenizer::intern_blob)
      .def("term_str", &Tokenizer::term_str)
      .def("num_terms", &Tokenizer::num_terms);
}
