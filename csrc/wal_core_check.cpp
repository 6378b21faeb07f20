// Stand-alone checker for csrc/wal_core.h: four threads write frames into
// two writers through both entry points (buffered append + commit, and
// write-through append_commit) while segments rotate; the files are read
// back and every frame is accounted for. Checks the order of syncs against
// closes (a rotation between the frames of a batch, a buffered frame flushed
// by another caller) and compares the table and the carry-less-multiply CRC
// paths with a bit-at-a-time reference. Meant to be
// built with the host compiler under -fsanitize=address,undefined and again
// under -fsanitize=thread (tests/test_wal_batch.py does that); it has no
// Python or GPU dependency.
//
//   wal_core_check [scratch-dir]

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "wal_core.h"

using namespace gdb_wal;

static std::atomic<int> failures{0};
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                      \
    }                                                                  \
  } while (0)

// ------------------------------------------------------------------- crc

static uint32_t crc32_bitwise(uint32_t crc, const uint8_t* p, size_t n) {
  crc = ~crc;
  for (size_t i = 0; i < n; i++) {
    crc ^= p[i];
    for (int k = 0; k < 8; k++) crc = (crc & 1) ? 0xEDB88320u ^ (crc >> 1) : crc >> 1;
  }
  return ~crc;
}

static void check_crc_one(const uint8_t* p, size_t n, uint32_t init) {
  const uint32_t want = crc32_bitwise(init, p, n);
  CHECK(crc32_table(init, p, n) == want);
  CHECK(crc32_update(init, p, n) == want);
  if (crc32_have_clmul()) CHECK(crc32_clmul(init, p, n) == want);
}

static void check_crc() {
  const size_t big = 300001;
  // exactly sized heap blocks, so a read past the end is an ASan report
  for (int fill = 0; fill < 3; fill++) {
    std::vector<uint8_t> buf(big + 16);
    uint32_t x = 0x9E3779B9u;
    for (auto& b : buf) {
      x = x * 1664525u + 1013904223u;
      b = fill == 0 ? (uint8_t)(x >> 24) : fill == 1 ? 0x00 : 0xFF;
    }
    for (size_t n = 0; n <= 300; n++) {
      std::vector<uint8_t> exact(buf.begin(), buf.begin() + n);
      check_crc_one(exact.data(), n, 0);
    }
    for (size_t n : {(size_t)4095, (size_t)4096, (size_t)4097, big}) {
      std::vector<uint8_t> exact(buf.begin(), buf.begin() + n);
      check_crc_one(exact.data(), n, 0);
      check_crc_one(exact.data(), n, 0xDEADBEEFu);
    }
    for (size_t off = 0; off < 16; off++) {
      std::vector<uint8_t> exact(buf.begin(), buf.begin() + off + 1000);
      check_crc_one(exact.data() + off, 1000, 0);
      check_crc_one(exact.data() + off, 77, 12345u);
    }
  }
  // chained updates equal one pass
  std::vector<uint8_t> buf(5000, 0xA5);
  CHECK(crc32_update(crc32_update(0, buf.data(), 1234), buf.data() + 1234, 3766) ==
        crc32_bitwise(0, buf.data(), 5000));
}

// ---------------------------------------------------------------- writers

constexpr int kWriters = 2;
constexpr int kThreads = 4;
constexpr int kFramesPerThread = 400;
constexpr uint64_t kSegmentBytes = 24 * 1024;

static size_t payload_len(uint64_t seq) { return (size_t)((seq * 131) % 700); }
static uint8_t payload_byte(uint64_t seq, size_t i) {
  return (uint8_t)(seq * 7 + i * 13 + (i >> 8));
}

struct Shard {
  WalWriter writer;
  std::vector<std::string> segments;   // guarded by seq_mu
};

static std::mutex seq_mu;          // guards next_seq, segment lists, rotation
static uint64_t next_seq = 1;
static std::string dir;

static std::string seg_path(int shard, uint64_t first_seq) {
  char name[64];
  std::snprintf(name, sizeof name, "/%020llu.s%d.wal",
                (unsigned long long)first_seq, shard);
  return dir + name;
}

static void maybe_rotate(Shard& sh, int idx, uint64_t size) {
  if (size < kSegmentBytes) return;
  std::lock_guard<std::mutex> g(seq_mu);
  if (sh.writer.segment_bytes() < kSegmentBytes) return;
  const std::string p = seg_path(idx, next_seq);
  sh.writer.rotate(p);
  sh.segments.push_back(p);
}

static void worker(Shard* shards, int tid) {
  std::vector<uint8_t> payload;
  for (int k = 0; k < kFramesPerThread; k++) {
    uint64_t seq;
    {
      std::lock_guard<std::mutex> g(seq_mu);
      seq = next_seq++;
    }
    const int idx = (int)((seq + (uint64_t)tid) % kWriters);
    Shard& sh = shards[idx];
    const uint64_t region = 4096 + (uint64_t)idx;
    payload.resize(payload_len(seq));
    for (size_t i = 0; i < payload.size(); i++) payload[i] = payload_byte(seq, i);
    uint64_t size;
    if (k % 3 == 0) {   // buffered path; every other one is left for a later
      sh.writer.append(region, seq, payload.data(), payload.size());   // call
      size = (k % 2 == 0) ? sh.writer.commit(false) : sh.writer.segment_bytes();
    } else {
      uint8_t hdr[kFrameHeaderBytes];
      frame_header(hdr, region, seq, payload.data(), payload.size());
      size = sh.writer.append_commit(hdr, payload.data(), payload.size(),
                                     k % 50 == 1);
    }
    maybe_rotate(sh, idx, size);
  }
}

static void check_writers() {
  Shard shards[kWriters];
  for (int i = 0; i < kWriters; i++) {
    const std::string p = seg_path(i, 1);
    shards[i].writer.open_segment(p);
    shards[i].segments.push_back(p);
  }
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; t++) threads.emplace_back(worker, shards, t);
  for (auto& t : threads) t.join();
  for (auto& sh : shards) {
    sh.writer.commit(true);
    sh.writer.close_segment();
  }

  std::map<uint64_t, int> seen;
  for (int i = 0; i < kWriters; i++) {
    CHECK(shards[i].segments.size() >= 3);   // rotation happened
    uint64_t prev_first = 0;
    for (size_t s = 0; s < shards[i].segments.size(); s++) {
      const std::string& path = shards[i].segments[s];
      const uint64_t first =
          std::strtoull(path.substr(path.rfind('/') + 1, 20).c_str(), nullptr, 10);
      CHECK(s == 0 || first >= prev_first);
      const std::vector<uint8_t> data = read_file(path);
      const std::vector<FrameView> frames = read_frames(data.data(), data.size());
      size_t bytes = 0;
      for (const auto& f : frames) {
        bytes += kFrameHeaderBytes + f.plen;
        seen[f.seq]++;
        CHECK(f.region == 4096 + (uint64_t)i);
        CHECK(f.plen == payload_len(f.seq));
        // what purge relies on: no frame of an earlier segment has a seq at
        // or above the name of a later one
        if (s + 1 < shards[i].segments.size()) {
          const std::string& nxt = shards[i].segments[s + 1];
          CHECK(f.seq < std::strtoull(
              nxt.substr(nxt.rfind('/') + 1, 20).c_str(), nullptr, 10));
        }
        bool same = f.plen == payload_len(f.seq);
        for (size_t b = 0; same && b < f.plen; b++)
          same = f.payload[b] == payload_byte(f.seq, b);
        CHECK(same);
      }
      CHECK(bytes == data.size());   // no torn or unreadable tail
      prev_first = first;
    }
  }
  const uint64_t total = (uint64_t)kThreads * kFramesPerThread;
  CHECK(seen.size() == total);
  for (uint64_t s = 1; s <= total; s++) CHECK(seen.count(s) && seen[s] == 1);

  // no open segment: both entry points refuse, append only buffers
  WalWriter closed;
  uint8_t hdr[kFrameHeaderBytes];
  frame_header(hdr, 1, 1, nullptr, 0);
  bool threw = false;
  try { closed.append_commit(hdr, nullptr, 0, false); } catch (const std::runtime_error&) { threw = true; }
  CHECK(threw);
  threw = false;
  try { closed.commit(false); } catch (const std::runtime_error&) { threw = true; }
  CHECK(threw);
  threw = false;
  try { closed.rotate(dir + "/no/such/dir/x.wal"); } catch (const std::runtime_error&) { threw = true; }
  CHECK(threw);
}

// ------------------------------------------------------------ sync order

static void put(WalWriter& w, uint64_t seq, bool sync) {
  const uint8_t payload[5] = {1, 2, 3, 4, 5};
  uint8_t hdr[kFrameHeaderBytes];
  frame_header(hdr, 7, seq, payload, sizeof payload);
  w.append_commit(hdr, payload, sizeof payload, sync);
}

// A batch of several frames syncs only behind its last one. Nothing it
// wrote may be left unsynced in a closed segment, and a commit(sync) must
// sync bytes that somebody else's write-through call flushed for it.
static void check_sync_order() {
  const size_t frame = kFrameHeaderBytes + 5;
  {   // rotation between the frames of one batch
    WalWriter w;
    w.open_segment(dir + "/sync_a.wal");
    put(w, 1, false);
    put(w, 2, false);
    put(w, 3, false);
    CHECK(w.unsynced_bytes() == 3 * frame && w.sync_count() == 0);
    w.rotate(dir + "/sync_b.wal", true);     // another worker's rotation
    CHECK(w.unsynced_bytes() == 0);          // old segment synced, then closed
    CHECK(w.sync_count() == 1);
    put(w, 4, true);                         // the batch's last frame
    CHECK(w.unsynced_bytes() == 0 && w.sync_count() == 2);
    // once a writer has synced, it never closes unsynced bytes, whatever
    // the closing call passes
    put(w, 5, false);
    w.rotate(dir + "/sync_c.wal");
    CHECK(w.unsynced_bytes() == 0 && w.sync_count() == 3);
    put(w, 6, false);
    w.close_segment();
    CHECK(w.sync_count() == 4);
    CHECK(read_frames(read_file(dir + "/sync_a.wal").data(), 3 * frame).size() == 3);
  }
  {   // buffered frame flushed by someone else's write-through call
    WalWriter w;
    w.open_segment(dir + "/sync_d.wal");
    const uint8_t payload[3] = {9, 9, 9};
    w.append(7, 1, payload, sizeof payload);    // thread A, general path
    put(w, 2, false);                           // thread B: flushes A's frame
    CHECK(w.unsynced_bytes() == kFrameHeaderBytes + 3 + frame);
    w.commit(true);                             // A's commit: buffer is empty
    CHECK(w.unsynced_bytes() == 0 && w.sync_count() == 1);
    w.commit(true);                             // nothing new: no second sync
    CHECK(w.sync_count() == 1);
    put(w, 3, true);
    CHECK(w.sync_count() == 2);
  }
  {   // a writer that never syncs does not start to on close
    WalWriter w;
    w.open_segment(dir + "/sync_e.wal");
    put(w, 1, false);
    w.commit(false);
    w.rotate(dir + "/sync_f.wal");
    w.close_segment();
    CHECK(w.sync_count() == 0);
  }
}

// Threads: batches of three frames on one writer, sync behind the last
// frame only, while every batch end may rotate. After each batch returns,
// whatever it wrote is synced: its frames are either in a segment that was
// synced before it was closed, or covered by the batch's own final sync.
static void check_sync_threads() {
  WalWriter w;
  std::mutex rot_mu;
  int seg = 0;
  std::atomic<uint64_t> seq{1};
  w.open_segment(dir + "/sync_t0.wal");
  auto body = [&](int tid) {
    for (int k = 0; k < 40; k++) {
      put(w, seq++, false);
      put(w, seq++, false);
      put(w, seq++, true);
      if ((k + tid) % 5 == 0) {
        std::lock_guard<std::mutex> g(rot_mu);
        char name[48];
        std::snprintf(name, sizeof name, "/sync_t%d.wal", ++seg);
        w.rotate(dir + name, true);
      }
    }
  };
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; t++) threads.emplace_back(body, t);
  for (auto& t : threads) t.join();
  w.close_segment(true);
  CHECK(w.unsynced_bytes() == 0);
  size_t frames = 0;
  for (int i = 0; i <= seg; i++) {
    char name[48];
    std::snprintf(name, sizeof name, "/sync_t%d.wal", i);
    const std::vector<uint8_t> data = read_file(dir + name);
    const size_t n = read_frames(data.data(), data.size()).size();
    CHECK(n * (kFrameHeaderBytes + 5) == data.size());
    frames += n;
  }
  CHECK(frames == (size_t)kThreads * 40 * 3);
}

int main(int argc, char** argv) {
  if (argc > 1) {
    dir = argv[1];
  } else {
    char tmpl[] = "/tmp/wal_core_check_XXXXXX";
    const char* d = mkdtemp(tmpl);
    if (!d) { std::perror("mkdtemp"); return 2; }
    dir = d;
  }
  check_crc();
  check_writers();
  check_sync_order();
  check_sync_threads();
  if (failures.load()) {
    std::printf("wal_core_check FAILED: %d\n", failures.load());
    return 1;
  }
  std::printf("wal_core_check ok\n");
  return 0;
}
