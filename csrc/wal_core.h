// WAL frame + segment-file core, Python-free (the pybind glue is in
// native.cpp; csrc/wal_core_check.cpp drives it stand-alone under the host
// sanitizers).
//
// Frame: [u32 len][u32 crc32][u64 region_id][u64 seq][payload], len = 16 +
// payload bytes, crc32 = zlib-compatible CRC over [region_id][seq][payload].
//
// WalWriter is internally synchronized: every entry point takes the writer's
// mutex, so callers need no lock of their own and may run without the GIL.
// Two ways in:
//   append() + commit()  — group commit: frames are buffered, commit() writes
//                          them with one write();
//   append_commit()      — write-through: the frame goes out with
//                          writev([24-byte header][payload]) straight from the
//                          caller's buffer (buffered frames first, so order is
//                          kept). The checksum is computed by the caller
//                          (frame_header) before the mutex is taken.
//
// Durability: the writer counts the bytes it has written and not yet
// fdatasync'ed, whichever entry point wrote them. commit(sync=true) syncs
// whenever that count is non-zero, also when another thread's write-through
// call has already flushed this caller's buffered frames; and no descriptor
// that has been asked to sync is ever closed (rotate, close_segment, the
// destructor) with unsynced bytes in it. A multi-frame batch that syncs only
// behind its last frame therefore stays durable when a rotation falls
// between its frames.
#pragma once

#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstring>
#include <fcntl.h>
#include <mutex>
#include <stdexcept>
#include <string>
#include <sys/uio.h>
#include <unistd.h>
#include <vector>

#if defined(__x86_64__) && (defined(__GNUC__) || defined(__clang__))
#define GDB_WAL_HAVE_CLMUL_BUILD 1
#include <immintrin.h>
#else
#define GDB_WAL_HAVE_CLMUL_BUILD 0
#endif

namespace gdb_wal {

// ------------------------------------------ crc32 (IEEE, zlib-compatible)

struct CrcTables {
  uint32_t t[8][256];
  CrcTables() {
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      t[0][i] = c;
    }
    for (int s = 1; s < 8; s++)
      for (uint32_t i = 0; i < 256; i++)
        t[s][i] = t[0][t[s - 1][i] & 0xFF] ^ (t[s - 1][i] >> 8);
  }
};

inline const CrcTables& crc_tables() {
  static const CrcTables tables;
  return tables;
}

// Slice-by-8 over the raw (pre-inverted) register.
inline uint32_t crc32_table_raw(uint32_t crc, const uint8_t* buf, size_t len) {
  const auto& T = crc_tables().t;
  while (len >= 8) {
    uint32_t lo, hi;
    std::memcpy(&lo, buf, 4);
    std::memcpy(&hi, buf + 4, 4);
    lo ^= crc;
    crc = T[7][lo & 0xFF] ^ T[6][(lo >> 8) & 0xFF] ^
          T[5][(lo >> 16) & 0xFF] ^ T[4][lo >> 24] ^
          T[3][hi & 0xFF] ^ T[2][(hi >> 8) & 0xFF] ^
          T[1][(hi >> 16) & 0xFF] ^ T[0][hi >> 24];
    buf += 8;
    len -= 8;
  }
  for (size_t i = 0; i < len; i++)
    crc = T[0][(crc ^ buf[i]) & 0xFF] ^ (crc >> 8);
  return crc;
}

inline uint32_t crc32_table(uint32_t crc, const uint8_t* buf, size_t len) {
  return ~crc32_table_raw(~crc, buf, len);
}

inline bool crc32_have_clmul() {
#if GDB_WAL_HAVE_CLMUL_BUILD
  static const bool have = __builtin_cpu_supports("pclmul") &&
                           __builtin_cpu_supports("sse4.1");
  return have;
#else
  return false;
#endif
}

#if GDB_WAL_HAVE_CLMUL_BUILD
// Carry-less-multiply folding (Gopal et al., "Fast CRC Computation for
// Generic Polynomials Using PCLMULQDQ Instruction", Intel 2009) for the
// bit-reflected polynomial 0x1DB710641. Consumes `len` bytes, len >= 64 and
// a multiple of 16, over the raw register; any alignment.
//   k1,k2 = x^(512+32), x^(512-32) mod P   fold four lanes across 64 bytes
//   k3,k4 = x^(128+32), x^(128-32) mod P   fold one lane across 16 bytes
//   k5    = x^64 mod P                     128 → 64 bits
//   P', mu                                 Barrett reduction 64 → 32 bits
#define GDB_WAL_CLMUL_FN __attribute__((target("pclmul,sse4.1"))) inline

GDB_WAL_CLMUL_FN __m128i clmul_load(const uint8_t* p) {
  return _mm_loadu_si128(reinterpret_cast<const __m128i*>(p));
}

// lane * x^shift mod P (shift per the constant pair k), plus the next 16
// input bytes
GDB_WAL_CLMUL_FN __m128i clmul_fold(__m128i lane, __m128i k, __m128i next) {
  const __m128i lo = _mm_clmulepi64_si128(lane, k, 0x00);
  const __m128i hi = _mm_clmulepi64_si128(lane, k, 0x11);
  return _mm_xor_si128(_mm_xor_si128(lo, hi), next);
}

GDB_WAL_CLMUL_FN uint32_t crc32_clmul_raw(uint32_t crc, const uint8_t* buf,
                                          size_t len) {
  const __m128i k1k2 = _mm_set_epi64x(0x01c6e41596, 0x0154442bd4);
  const __m128i k3k4 = _mm_set_epi64x(0x00ccaa009e, 0x01751997d0);
  const __m128i k5 = _mm_set_epi64x(0, 0x0163cd6124);
  const __m128i poly_mu = _mm_set_epi64x(0x01f7011641, 0x01db710641);
  const __m128i low32 = _mm_set_epi32(0, ~0, 0, ~0);
  __m128i a = _mm_xor_si128(clmul_load(buf), _mm_cvtsi32_si128((int)crc));
  __m128i b = clmul_load(buf + 16), c = clmul_load(buf + 32), d = clmul_load(buf + 48);
  buf += 64;
  len -= 64;
  while (len >= 64) {
    a = clmul_fold(a, k1k2, clmul_load(buf));
    b = clmul_fold(b, k1k2, clmul_load(buf + 16));
    c = clmul_fold(c, k1k2, clmul_load(buf + 32));
    d = clmul_fold(d, k1k2, clmul_load(buf + 48));
    buf += 64;
    len -= 64;
  }
  a = clmul_fold(a, k3k4, b);
  a = clmul_fold(a, k3k4, c);
  a = clmul_fold(a, k3k4, d);
  while (len >= 16) {
    a = clmul_fold(a, k3k4, clmul_load(buf));
    buf += 16;
    len -= 16;
  }
  // 128 → 64 bits
  __m128i t = _mm_clmulepi64_si128(a, k3k4, 0x10);
  a = _mm_xor_si128(_mm_srli_si128(a, 8), t);
  t = _mm_srli_si128(a, 4);
  a = _mm_clmulepi64_si128(_mm_and_si128(a, low32), k5, 0x00);
  a = _mm_xor_si128(a, t);
  // Barrett: 64 → 32 bits
  t = _mm_clmulepi64_si128(_mm_and_si128(a, low32), poly_mu, 0x10);
  t = _mm_clmulepi64_si128(_mm_and_si128(t, low32), poly_mu, 0x00);
  a = _mm_xor_si128(a, t);
  return (uint32_t)_mm_extract_epi32(a, 1);
}
#endif

// Folding for the 16-byte-multiple prefix of buffers >= 64 bytes, slice-by-8
// for the tail. Throws on a CPU without pclmul + sse4.1.
inline uint32_t crc32_clmul(uint32_t crc, const uint8_t* buf, size_t len) {
#if GDB_WAL_HAVE_CLMUL_BUILD
  if (!crc32_have_clmul())
    throw std::runtime_error("crc32: this CPU has no pclmul + sse4.1");
  crc = ~crc;
  if (len >= 64) {
    const size_t head = len & ~(size_t)15;
    crc = crc32_clmul_raw(crc, buf, head);
    buf += head;
    len -= head;
  }
  return ~crc32_table_raw(crc, buf, len);
#else
  (void)crc; (void)buf; (void)len;
  throw std::runtime_error("crc32: built without pclmul support");
#endif
}

// Process-wide switch of the "auto" path: set = always the table (for
// measurements; see _native.crc32_force_table).
inline std::atomic<bool>& crc32_force_table_flag() {
  static std::atomic<bool> force{false};
  return force;
}

inline uint32_t crc32_update(uint32_t crc, const uint8_t* buf, size_t len) {
  if (len >= 64 && crc32_have_clmul() &&
      !crc32_force_table_flag().load(std::memory_order_relaxed))
    return crc32_clmul(crc, buf, len);
  return crc32_table(crc, buf, len);
}

// ---------------------------------------------------------------- frames

constexpr size_t kFrameHeaderBytes = 24;

// [u32 len][u32 crc][u64 region][u64 seq] of the frame around `payload`.
inline void frame_header(uint8_t out[kFrameHeaderBytes], uint64_t region_id,
                         uint64_t seq, const uint8_t* payload, size_t plen) {
  if (plen > 0xFFFFFFFFull - 16)
    throw std::runtime_error("wal: payload too large for one frame");
  const uint32_t body_len = 16 + static_cast<uint32_t>(plen);
  std::memcpy(out, &body_len, 4);
  std::memcpy(out + 8, &region_id, 8);
  std::memcpy(out + 16, &seq, 8);
  uint32_t crc = crc32_update(0, out + 8, 16);
  crc = crc32_update(crc, payload, plen);
  std::memcpy(out + 4, &crc, 4);
}

// ---------------------------------------------------------------- writer

class WalWriter {
 public:
  WalWriter() = default;
  WalWriter(const WalWriter&) = delete;
  WalWriter& operator=(const WalWriter&) = delete;
  ~WalWriter() {
    try { close_segment(); } catch (...) {}
  }

  void open_segment(const std::string& path) {
    std::lock_guard<std::mutex> g(mu_);
    open_locked(path);
  }

  // `sync`: fdatasync what the segment still holds unsynced before closing
  // (implied once any call on this writer has asked for sync).
  void close_segment(bool sync = false) {
    std::lock_guard<std::mutex> g(mu_);
    close_locked(sync);
  }

  // Close the current segment and open `path` under one hold of the mutex:
  // a concurrent writer sees the old descriptor or the new one, never none.
  // Frames still buffered stay buffered and go to the new segment. The old
  // segment is synced before it is closed, as in close_segment.
  void rotate(const std::string& path, bool sync = false) {
    std::lock_guard<std::mutex> g(mu_);
    open_locked(path, sync);
  }

  // Buffer one frame (commit() writes it). Checksum first, lock second.
  void append(uint64_t region_id, uint64_t seq, const uint8_t* payload,
              size_t plen) {
    uint8_t hdr[kFrameHeaderBytes];
    frame_header(hdr, region_id, seq, payload, plen);
    std::lock_guard<std::mutex> g(mu_);
    const size_t off = buf_.size();
    buf_.resize(off + kFrameHeaderBytes + plen);
    std::memcpy(buf_.data() + off, hdr, kFrameHeaderBytes);
    if (plen) std::memcpy(buf_.data() + off + kFrameHeaderBytes, payload, plen);
  }

  // Write buffered frames; optionally fdatasync. Returns the segment size.
  uint64_t commit(bool sync) {
    std::lock_guard<std::mutex> g(mu_);
    if (fd_ < 0) throw std::runtime_error("wal: no open segment");
    flush_locked();
    if (sync) sync_locked();
    return seg_bytes_;
  }

  // Write one frame through: buffered frames first, then `hdr` (from
  // frame_header) and the payload with writev, no copy. Returns the segment
  // size.
  uint64_t append_commit(const uint8_t hdr[kFrameHeaderBytes],
                         const uint8_t* payload, size_t plen, bool sync) {
    std::lock_guard<std::mutex> g(mu_);
    if (fd_ < 0) throw std::runtime_error("wal: no open segment");
    flush_locked();
    size_t done = 0;
    const size_t total = kFrameHeaderBytes + plen;
    while (done < total) {
      struct iovec iov[2];
      int cnt = 0;
      if (done < kFrameHeaderBytes) {
        iov[cnt].iov_base = const_cast<uint8_t*>(hdr) + done;
        iov[cnt].iov_len = kFrameHeaderBytes - done;
        cnt++;
        if (plen) {
          iov[cnt].iov_base = const_cast<uint8_t*>(payload);
          iov[cnt].iov_len = plen;
          cnt++;
        }
      } else {
        const size_t poff = done - kFrameHeaderBytes;
        iov[cnt].iov_base = const_cast<uint8_t*>(payload) + poff;
        iov[cnt].iov_len = plen - poff;
        cnt++;
      }
      const ssize_t w = ::writev(fd_, iov, cnt);
      if (w < 0) {
        if (errno == EINTR) continue;
        // a torn frame fails its checksum on replay; account for its bytes
        seg_bytes_ += done;
        unsynced_ += done;
        throw std::runtime_error(std::string("wal write failed: ") +
                                 strerror(errno));
      }
      done += static_cast<size_t>(w);
    }
    seg_bytes_ += total;
    unsynced_ += total;
    if (sync) sync_locked();
    return seg_bytes_;
  }

  uint64_t segment_bytes() {
    std::lock_guard<std::mutex> g(mu_);
    return seg_bytes_;
  }

  // Bytes written to the open segment and not yet fdatasync'ed.
  uint64_t unsynced_bytes() {
    std::lock_guard<std::mutex> g(mu_);
    return unsynced_;
  }

  // fdatasync calls made so far (for checks of the sync ordering).
  uint64_t sync_count() {
    std::lock_guard<std::mutex> g(mu_);
    return sync_count_;
  }

 private:
  // A sync failure throws and leaves the segment open.
  void close_locked(bool sync) {
    if (fd_ < 0) return;
    if (sync) sync_locked();
    else if (want_sync_ && unsynced_) sync_locked();
    ::close(fd_);
    fd_ = -1;
    unsynced_ = 0;
  }

  void open_locked(const std::string& path, bool sync = false) {
    const int fd = ::open(path.c_str(), O_CREAT | O_WRONLY | O_APPEND, 0644);
    if (fd < 0)
      throw std::runtime_error("wal open failed: " + path + ": " + strerror(errno));
    try {
      close_locked(sync);
    } catch (...) {
      ::close(fd);
      throw;
    }
    fd_ = fd;
    seg_bytes_ = static_cast<uint64_t>(::lseek(fd_, 0, SEEK_END));
  }

  void flush_locked() {
    const uint8_t* p = buf_.data();
    size_t left = buf_.size();
    while (left) {
      const ssize_t w = ::write(fd_, p, left);
      if (w < 0) {
        if (errno == EINTR) continue;
        throw std::runtime_error(std::string("wal write failed: ") + strerror(errno));
      }
      p += w;
      left -= static_cast<size_t>(w);
    }
    seg_bytes_ += buf_.size();
    unsynced_ += buf_.size();
    buf_.clear();
  }

  // fdatasync if anything written is still unsynced; remembers that this
  // writer runs with sync.
  void sync_locked() {
    want_sync_ = true;
    if (unsynced_ == 0) return;
    if (::fdatasync(fd_) != 0)
      throw std::runtime_error(std::string("wal fdatasync failed: ") + strerror(errno));
    sync_count_++;
    unsynced_ = 0;
  }

  std::mutex mu_;
  int fd_ = -1;
  uint64_t seg_bytes_ = 0;
  uint64_t unsynced_ = 0;     // written to fd_, not yet fdatasync'ed
  uint64_t sync_count_ = 0;
  bool want_sync_ = false;    // some call asked for sync: never close unsynced
  std::vector<uint8_t> buf_;
};

// One parsed frame of a segment image.
struct FrameView {
  uint64_t region, seq;
  const uint8_t* payload;
  size_t plen;
};

// Walk the frames of a segment image; stops at the first corrupt or
// truncated frame (torn tail after a crash).
inline std::vector<FrameView> read_frames(const uint8_t* data, size_t n) {
  std::vector<FrameView> out;
  size_t off = 0;
  while (off + 8 <= n) {
    uint32_t body_len, crc;
    std::memcpy(&body_len, data + off, 4);
    std::memcpy(&crc, data + off + 4, 4);
    if (body_len < 16 || off + 8 + (size_t)body_len > n) break;
    const uint8_t* body = data + off + 8;
    if (crc32_update(0, body, body_len) != crc) break;
    FrameView f;
    std::memcpy(&f.region, body, 8);
    std::memcpy(&f.seq, body + 8, 8);
    f.payload = body + 16;
    f.plen = body_len - 16;
    out.push_back(f);
    off += 8 + (size_t)body_len;
  }
  return out;
}

// Whole file into memory (what a short read returned so far on error).
inline std::vector<uint8_t> read_file(const std::string& path) {
  const int fd = ::open(path.c_str(), O_RDONLY);
  if (fd < 0) throw std::runtime_error("wal open failed: " + path);
  const off_t sz = ::lseek(fd, 0, SEEK_END);
  ::lseek(fd, 0, SEEK_SET);
  std::vector<uint8_t> data(sz > 0 ? (size_t)sz : 0);
  size_t got = 0;
  while (got < data.size()) {
    const ssize_t r = ::read(fd, data.data() + got, data.size() - got);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) break;
    got += (size_t)r;
  }
  ::close(fd);
  data.resize(got);
  return data;
}

}  // namespace gdb_wal
