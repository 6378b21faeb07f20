// Stand-alone checker for csrc/ingest_core.h: feeds the parse/route core
// fixed and randomised line-protocol batches and cross-checks the fused pass
// against a plain parse of the same bytes. Meant to be built with the host
// compiler and -fsanitize=address,undefined (tests/test_ingest_fused.py does
// that); it has no Python or GPU dependency.

#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "ingest_core.h"

using namespace gdb_ingest;

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                      \
    }                                                                  \
  } while (0)

struct Plain {
  std::vector<int32_t> series;
  std::vector<int64_t> ts;
  std::vector<double> cols;   // [F, cap]
  ParseSink sink;
  size_t n = 0, cap = 0;
};

static void plain_parse(LineCore& core, const std::string& data, Plain& out) {
  out.cap = LineCore::count_lines(data.data(), data.size());
  const size_t F = core.num_fields();
  out.series.assign(out.cap + 1, -1);
  out.ts.assign(out.cap + 1, -1);
  out.cols.assign(F * out.cap + 1, 0.0);
  out.sink.series = out.series.data();
  out.sink.ts = out.ts.data();
  out.sink.cap = out.cap;
  out.sink.col.resize(F);
  for (size_t c = 0; c < F; c++) out.sink.col[c] = out.cols.data() + c * out.cap;
  out.n = core.parse(data.data(), data.size(), out.sink);
}

static bool same_double(double a, double b) {
  return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, 8) == 0;
}

static int64_t floor_ms(int64_t ns, int64_t scale) {
  const int64_t t = (int64_t)((uint64_t)ns * (uint64_t)scale);
  int64_t q = t / 1000000;
  if (t % 1000000 < 0) q--;
  return q;
}

static void fixed_cases() {
  LineCore core;
  const std::string data =
      "cpu,hostname=h1,region=r f1=1.25,f2=-3i,f3=2e3 1451606400000000000\n"
      "# comment\n\n"
      "cpu,hostname=h2,region=r f1=7,f2=9u,b=t,s=\"x,y\" -1500000\n"
      "bad-line-no-space\n"
      "cpu,hostname=h1,region=r f2=1i";
  Plain p;
  plain_parse(core, data, p);
  CHECK(p.cap == 4 && p.n == 3);
  CHECK(core.num_series() == 2 && core.num_fields() == 5);
  CHECK(p.series[0] == 0 && p.series[1] == 1 && p.series[2] == 0);
  CHECK(p.ts[0] == 1451606400000000000LL && p.ts[1] == -1500000 && p.ts[2] == 0);
  CHECK(p.sink.new_tagsets.size() == 2);
  // fields f1,f2,f3 were new in this batch: they live in sink.extra
  CHECK(p.sink.col.size() == 5);
  CHECK(p.sink.col[0][0] == 1.25 && p.sink.col[1][0] == -3.0 && p.sink.col[2][0] == 2000.0);
  CHECK(p.sink.col[0][1] == 7.0 && p.sink.col[1][1] == 9.0 && std::isnan(p.sink.col[2][1]));
  CHECK(p.sink.col[3][1] == 1.0 && std::isnan(p.sink.col[4][1]));
  CHECK(std::isnan(p.sink.col[0][2]) && p.sink.col[1][2] == 1.0);
  CHECK(floor_ms(-1, 1) == -1 && floor_ms(-1000000, 1) == -1 && floor_ms(-1000001, 1) == -2);
  CHECK(hash64("abc", 3) != hash64("abd", 3));
  CHECK(hash64("", 0) == hash64("x", 0));

  // empty and comment-only input
  Plain e;
  plain_parse(core, std::string(), e);
  CHECK(e.n == 0);
  plain_parse(core, std::string("#x\n\n"), e);
  CHECK(e.n == 0);
}

static std::string make_batch(std::mt19937_64& rng, int rows, int n_hosts,
                              const std::vector<std::string>& fields,
                              bool noise) {
  std::string s;
  for (int i = 0; i < rows; i++) {
    const int h = (int)(rng() % n_hosts);
    s += "cpu,hostname=host_" + std::to_string(h) + ",region=eu-" +
         std::to_string(h % 5) + ",rack=" + std::to_string(h * 7 % 97) + " ";
    bool first = true;
    for (const auto& f : fields) {
      if (noise && rng() % 10 == 0) continue;
      if (!first) s += ",";
      first = false;
      s += f + "=";
      switch (rng() % 5) {
        case 0: s += std::to_string((int64_t)(rng() % 2000) - 1000) + "i"; break;
        case 1: s += (rng() % 2) ? "t" : "F"; break;
        default:
          s += std::to_string((int64_t)(rng() % 200000) - 100000) + "." +
               std::to_string(rng() % 1000000);
      }
    }
    if (first) s += fields[0] + "=1";
    if (!noise || rng() % 20 != 0)
      s += " " + std::to_string((int64_t)(rng() % 4000000000000ULL) - 2000000000000LL);
    if (i + 1 < rows || rng() % 2) s += "\n";
    if (noise && rng() % 50 == 0) s += "# note\n\n";
    if (noise && rng() % 200 == 0) s += "garbage\n";
  }
  return s;
}

// fused pass vs plain parse of the same bytes by a twin core
static void fused_cases() {
  std::mt19937_64 rng(20261020);
  const std::vector<std::string> fields = {"usage_user", "usage_system", "usage_idle", "n"};
  LineCore core, twin;
  const int n_hosts = 4000, R = 4;
  // routing: warm both cores, then route host h to region h % R
  {
    std::string warm;
    for (int h = 0; h < n_hosts; h++)
      warm += "cpu,hostname=host_" + std::to_string(h) + ",region=eu-" +
              std::to_string(h % 5) + ",rack=" + std::to_string(h * 7 % 97) +
              " usage_user=1,usage_system=2,usage_idle=3,n=4i 1\n";
    Plain a, b;
    plain_parse(core, warm, a);
    plain_parse(twin, warm, b);
    CHECK(a.n == (size_t)n_hosts && core.num_series() == (size_t)n_hosts);
    CHECK(core.intern_capacity() >= 8192);   // 1024 → grown by rehash
  }
  std::vector<int32_t> sid_region(n_hosts), sid_local(n_hosts);
  for (int s = 0; s < n_hosts; s++) { sid_region[s] = s % R; sid_local[s] = s / R; }
  // table order: usage_idle, (absent), n, usage_user, usage_system
  const std::vector<int64_t> fmap = {2, -1, 3, 0, 1};
  const int nf = (int)fmap.size();
  const std::string suffix = ", \"fields\": [], \"strs\": [], \"bins\": [], \"new_series\": []}";
  std::vector<char> stage;

  for (int round = 0; round < 40; round++) {
    const int rows = round == 0 ? 1 : (int)(1 + rng() % 700);
    const bool noise = round % 2 == 1;
    const int64_t scale = (round % 3 == 0) ? 1000 : 1;
    const std::string data = make_batch(rng, rows, n_hosts, fields, noise);
    FusedResult res;
    fused_ingest(core, data.data(), data.size(), sid_region.data(), sid_local.data(),
                 sid_region.size(), fmap.data(), nf, 4, R, suffix, true, scale,
                 stage.data(), stage.size(), res);
    if (res.status == FUSED_GROW) {
      CHECK(res.need_bytes > stage.size());
      stage.assign(res.need_bytes, (char)0x5A);   // exact fit: ASan guards the end
      res = FusedResult();
      fused_ingest(core, data.data(), data.size(), sid_region.data(), sid_local.data(),
                   sid_region.size(), fmap.data(), nf, 4, R, suffix, true, scale,
                   stage.data(), stage.size(), res);
    }
    CHECK(res.status == FUSED_OK);
    Plain p;
    plain_parse(twin, data, p);
    CHECK(res.n == p.n);
    if (res.status != FUSED_OK || res.n != p.n) continue;
    const size_t n = p.n;
    const StageLayout L(n, (size_t)nf);
    CHECK(L.total <= stage.size());
    const int64_t* ts = reinterpret_cast<const int64_t*>(stage.data() + L.ts);
    const double* f = reinterpret_cast<const double*>(stage.data() + L.fields);
    const int64_t* dst = reinterpret_cast<const int64_t*>(stage.data() + L.dst_off);
    const int32_t* se = reinterpret_cast<const int32_t*>(stage.data() + L.series);
    const int32_t* rg = reinterpret_cast<const int32_t*>(stage.data() + L.region);
    std::vector<int64_t> cnt(R, 0);
    for (size_t i = 0; i < n; i++) {
      const int32_t sid = p.series[i];
      CHECK(rg[i] == sid % R && se[i] == sid / R);
      CHECK(dst[i] == cnt[rg[i]]);
      cnt[rg[i]]++;
      CHECK(ts[i] == floor_ms(p.ts[i], scale));
      for (int t = 0; t < nf; t++) {
        const double want = fmap[t] < 0 ? std::nan("") : p.sink.col[fmap[t]][i];
        CHECK(same_double(f[(size_t)t * n + i], want));
      }
    }
    size_t wal = 0;
    for (int r = 0; r < R; r++) {
      CHECK(res.counts[r] == cnt[r]);
      const size_t len = res.wal_off[r + 1] - res.wal_off[r];
      if (cnt[r] == 0) { CHECK(len == 0); continue; }
      uint32_t hl;
      std::memcpy(&hl, res.wal.data() + res.wal_off[r], 4);
      CHECK(len == 4 + hl + (size_t)cnt[r] * (12 + 8 * nf));
      wal += len;
    }
    CHECK(wal == res.wal.size());
  }

  // fallbacks: new series, new field, unrouted sid, too many regions
  {
    FusedResult res;
    const std::string d = "cpu,hostname=brand_new usage_user=1 5\n";
    fused_ingest(core, d.data(), d.size(), sid_region.data(), sid_local.data(),
                 sid_region.size(), fmap.data(), nf, 4, R, suffix, true, 1,
                 stage.data(), stage.size(), res);
    CHECK(res.status == FUSED_SLOW && res.n == 1 && res.sink.new_tagsets.size() == 1);
    CHECK(res.sink.col[0][0] == 1.0 && std::isnan(res.sink.col[1][0]));
  }
  {
    FusedResult res;
    const std::string d = "cpu,hostname=host_1,region=eu-1,rack=7 usage_user=1,fresh=2 5\n";
    fused_ingest(core, d.data(), d.size(), sid_region.data(), sid_local.data(),
                 sid_region.size(), fmap.data(), nf, 4, R, suffix, true, 1,
                 stage.data(), stage.size(), res);
    CHECK(res.status == FUSED_SLOW && res.n == 1 && core.num_fields() == 5);
    CHECK(res.sink.col.size() == 5 && res.sink.col[4][0] == 2.0);
  }
  {
    FusedResult res;
    const std::string d = "cpu,hostname=host_2,region=eu-2,rack=14 usage_user=1 5\n";
    sid_region[2] = -1;
    fused_ingest(core, d.data(), d.size(), sid_region.data(), sid_local.data(),
                 sid_region.size(), fmap.data(), nf, 5, R, suffix, true, 1,
                 stage.data(), stage.size(), res);
    CHECK(res.status == FUSED_SLOW && res.n == 1);
    FusedResult res2;
    fused_ingest(core, d.data(), d.size(), sid_region.data(), sid_local.data(),
                 sid_region.size(), fmap.data(), nf, 5, kMaxPackedRegions + 1, suffix,
                 true, 1, stage.data(), stage.size(), res2);
    CHECK(res2.status == FUSED_SLOW && res2.n == 1);
  }
}

int main() {
  fixed_cases();
  fused_cases();
  if (failures) {
    std::printf("ingest_core_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("ingest_core_check ok\n");
  return 0;
}
