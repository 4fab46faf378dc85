// kubebrain_amd/csrc/splan_hostcheck.cc — stand-alone CPU check of the batched
// stream read's arithmetic (splan.h) against naive loops: the window end, the
// delta end rule, the tile map (every row of both segments in exactly one
// tile, whole ballot words per tile) and the cut (largest n under max_kvs,
// the caller's buffer and the arena, plus the KB_ENOBUF size). At the edges:
// window = 64, segments of 0 / 63 / 64 / 65 rows, cap at a record's last
// byte, max_kvs = 1; then seeded random cases.
// No HIP, no store; meant to be built with sanitizers:
//   make -C kubebrain_amd/csrc stream-hostcheck        (plain)
//   make -C kubebrain_amd/csrc stream-hostcheck-asan   (-fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "splan.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

using namespace kbstream;

static int64_t g_cases = 0;

// one window over base rows [lo, hi) and delta rows [dlo, dhi); key_lb = where
// the key of base row e starts in the delta run
static int check_window(int64_t lo, int64_t hi, int64_t dlo, int64_t dhi,
                        int64_t W, int64_t key_lb) {
  ++g_cases;
  int64_t e = lo;  // naive: step row by row
  for (int64_t k = 0; k < W && e < hi; ++k) ++e;
  CHECK(WindowEnd(lo, hi, W) == e);
  CHECK(e - lo <= W && e >= lo && (hi <= lo || e <= hi));
  int64_t want = dhi < dlo ? dlo : dhi;
  if (e < hi) {
    want = key_lb;
    if (want < dlo) want = dlo;
    if (want > (dhi < dlo ? dlo : dhi)) want = dhi < dlo ? dlo : dhi;
  }
  const int64_t dhiw = DeltaEnd(e, hi, dlo, dhi, key_lb);
  CHECK(dhiw == want && dhiw >= dlo);
  // the tile map covers both segments exactly once, in order, in whole words
  const uint64_t total = SegTiles(e - lo) + SegTiles(dhiw - dlo);
  std::vector<int> bhit((size_t)(e - lo)), dhit((size_t)(dhiw - dlo));
  int64_t prev_run = 0, prev_r1 = lo;
  for (uint64_t t = 0; t < total; ++t) {
    const Tile tl = MapTile(lo, e, dlo, dhiw, t);
    const int64_t s0 = tl.run ? dlo : lo, s1 = tl.run ? dhiw : e;
    CHECK(tl.r0 < tl.r1 && tl.r0 >= s0 && tl.r1 <= s1);
    CHECK((tl.r0 - s0) % kTile == 0 && tl.r1 - tl.r0 <= kTile);
    CHECK(tl.run >= prev_run);
    if (tl.run != prev_run) { prev_run = tl.run; prev_r1 = dlo; }
    CHECK(tl.r0 == prev_r1);
    prev_r1 = tl.r1;
    for (int64_t r = tl.r0; r < tl.r1; ++r)
      ++(tl.run ? dhit : bhit)[(size_t)(r - s0)];
  }
  for (int h : bhit) CHECK(h == 1);
  for (int h : dhit) CHECK(h == 1);
  CHECK(SegWords(e - lo) == (e - lo + 63) / 64);
  return 0;
}

static int check_cut(const std::vector<uint64_t>& sizes, uint64_t max_kvs,
                     uint64_t cap, uint64_t arena) {
  ++g_cases;
  const uint64_t lim = CutLimit(cap, arena);
  CHECK(cap < 4 ? lim == 0 : (lim <= cap - 4 && lim <= arena));
  // naive: try every n, keep the largest that respects the three bounds
  uint64_t best = 0, best_bytes = 0, acc = 0;
  for (size_t n = 1; n <= sizes.size(); ++n) {
    acc += sizes[n - 1];
    if (n <= max_kvs && cap >= 4 && 4 + acc <= cap && acc <= arena) {
      best = n;
      best_bytes = acc;
    }
  }
  const Cut c = CutTable(sizes.data(), sizes.size(), max_kvs, lim);
  CHECK(c.n == best && c.bytes == best_bytes);
  // Fits() marks exactly the prefix [0, n)
  uint64_t off = 0;
  for (size_t j = 0; j < sizes.size(); ++j) {
    CHECK(Fits(j, off, sizes[j], max_kvs, lim) == (j < c.n));
    off += sizes[j];
  }
  if (!sizes.empty() && c.n == 0 && sizes[0] <= arena && max_kvs > 0) {
    // the buffer is what stops the first record: the ENOBUF size admits it
    const uint64_t need = EnobufSize(sizes[0]);
    CHECK(need > cap);
    CHECK(CutTable(sizes.data(), sizes.size(), max_kvs, CutLimit(need, arena)).n >= 1);
  }
  return 0;
}

int main() {
  CHECK(ClampWindow(0) == 64 && ClampWindow(64) == 64 && ClampWindow(127) == 64 &&
        ClampWindow(192) == 192 && ClampWindow(1ll << 40) == kMaxWindow);
  CHECK(ResolveMaxKvs(0, 65536) == 65536 && ResolveMaxKvs(-5, 9) == 9 &&
        ResolveMaxKvs(7, 9) == 7 && ResolveMaxKvs(10, 9) == 9 &&
        ResolveMaxKvs(1, 9) == 1);
  CHECK(ClampLo(-1, 5) == 0 && ClampLo(9, 5) == 5 && ClampHi(3, 2, 5) == 3 &&
        ClampHi(3, 9, 5) == 5);
  const int64_t lens[] = {0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049};
  for (int64_t W : {64ll, 128ll, 192ll, 1024ll, 4096ll})
    for (int64_t lo : {0ll, 1ll, 63ll, 64ll, 1000ll})
      for (int64_t bl : lens)
        for (int64_t dlo : {0ll, 5ll})
          for (int64_t dl : lens)
            for (int64_t klb : {dlo - 1, dlo, dlo + dl / 2, dlo + dl, dlo + dl + 3})
              if (check_window(lo, lo + bl, dlo, dlo + dl, W, klb)) return 1;
  // inverted bounds hold no row
  if (check_window(10, 4, 7, 2, 64, 3)) return 1;
  // the cut: cap at a record's last byte, one short of it and one past it
  const std::vector<uint64_t> sizes = {40, 16, 4113, 17, 600, 31};
  uint64_t acc = 0;
  for (size_t k = 0; k <= sizes.size(); ++k) {
    for (uint64_t mk : {1ull, 2ull, 6ull, 7ull, 65536ull})
      for (int64_t dcap : {-1, 0, 1})
        for (uint64_t arena : {15ull, 40ull, 56ull, 4200ull, 1ull << 30}) {
          const int64_t cap = 4 + (int64_t)acc + dcap;
          if (check_cut(sizes, mk, (uint64_t)cap, arena)) return 1;
        }
    if (k < sizes.size()) acc += sizes[k];
  }
  for (uint64_t cap = 0; cap < 8; ++cap)
    if (check_cut(sizes, 3, cap, 1 << 20)) return 1;
  if (check_cut({}, 5, 100, 100)) return 1;
  srand(7);
  for (int it = 0; it < 2000; ++it) {
    std::vector<uint64_t> s((size_t)(rand() % 40));
    uint64_t sum = 0;
    for (auto& x : s) { x = 16 + (uint64_t)(rand() % 700); sum += x; }
    if (check_cut(s, 1 + (uint64_t)(rand() % 45), (uint64_t)rand() % (sum + 40),
                  (uint64_t)rand() % (sum + 40)))
      return 1;
    const int64_t lo = rand() % 5000, bl = rand() % 9000, dlo = rand() % 300,
                  dl = rand() % 3000;
    if (check_window(lo, lo + bl, dlo, dlo + dl, 64 * (1 + rand() % 40),
                     dlo - 2 + rand() % (dl + 5)))
      return 1;
  }
  printf("splan hostcheck: %lld cases ok\n", (long long)g_cases);
  return 0;
}
