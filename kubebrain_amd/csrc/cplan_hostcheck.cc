// kubebrain_amd/csrc/cplan_hostcheck.cc — stand-alone CPU check of the batched
// Count's tile map (cplan.h) against naive enumeration: every row of every
// segment lies in exactly one tile, no tile is empty, no tile crosses a
// segment, and tiles come in segment order. Exhaustively for one query with
// every bound in [0, 5] and two queries with every bound in [0, 3] (empty
// and inverted segments included) at T = 1 .. 4 (the map itself takes any T
// >= 1), then segment lengths around the tile edges at T = 64, 128, 4096,
// then seeded random bounds up to 1024 queries at real tile sizes.
// No HIP, no store; meant to be built with sanitizers:
//   make -C kubebrain_amd/csrc count-hostcheck        (plain)
//   make -C kubebrain_amd/csrc count-hostcheck-asan   (-fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cplan.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

using namespace kbcount;

static int64_t g_cases = 0;

// bounds = 4 per query {lo, hi, dlo, dhi}; rows of a run are < run_rows
static int check_case(const std::vector<int64_t>& bounds, int64_t T,
                      int64_t run_rows) {
  const int nq = (int)(bounds.size() / 4), nseg = 2 * nq;
  ++g_cases;
  // arrays of exactly the used size, so that an overrun is a sanitizer report
  std::vector<uint64_t> pfx((size_t)nseg + 1);
  const uint64_t total = BuildPrefix(bounds.data(), nq, T, pfx.data());
  CHECK(pfx[0] == 0 && pfx[(size_t)nseg] == total);
  // naive: tiles and rows per segment
  uint64_t want_tiles = 0, want_rows = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t lo = SegLo(bounds.data(), s), hi = SegHi(bounds.data(), s);
    uint64_t tiles = 0;
    for (int64_t r = lo; r < hi; r += T) ++tiles;
    CHECK(pfx[(size_t)s + 1] - pfx[(size_t)s] == tiles);
    CHECK(SegTiles(lo, hi, T) == tiles);
    CHECK(SegRows(lo, hi) == (hi > lo ? hi - lo : 0));
    want_tiles += tiles;
    want_rows += (uint64_t)SegRows(lo, hi);
  }
  CHECK(total == want_tiles);
  CHECK(want_rows <= total * (uint64_t)T);
  CHECK(total <= want_rows / (uint64_t)T + (uint64_t)nseg);
  // cover[run][row] per query would be large: walk the tiles in id order and
  // check that they enumerate each segment's rows front to back, gap-free
  int prev_seg = -1;
  int64_t next_row = 0;
  uint64_t rows = 0;
  for (uint64_t t = 0; t < total; ++t) {
    const Tile tl = MapTile(bounds.data(), pfx.data(), nseg, t, T);
    const int s = tl.query * 2 + tl.run;
    CHECK(tl.query >= 0 && tl.query < nq && (tl.run == 0 || tl.run == 1));
    CHECK(s == FindSeg(pfx.data(), nseg, t));
    const int64_t lo = SegLo(bounds.data(), s), hi = SegHi(bounds.data(), s);
    CHECK(tl.hi == hi);
    CHECK(tl.r0 < tl.r1);                              // no empty tile
    CHECK(tl.r0 >= lo && tl.r1 <= hi);                 // inside its segment
    CHECK(tl.r1 - tl.r0 <= T);
    CHECK(tl.r0 >= 0 && tl.r1 <= run_rows);
    if (s != prev_seg) {
      CHECK(s > prev_seg);                             // segment order
      // the segment before must have been finished, skipped ones were empty
      if (prev_seg >= 0) CHECK(next_row == SegHi(bounds.data(), prev_seg));
      for (int k = prev_seg + 1; k < s; ++k)
        CHECK(SegRows(SegLo(bounds.data(), k), SegHi(bounds.data(), k)) == 0);
      CHECK(tl.r0 == lo);
      prev_seg = s;
    } else {
      CHECK(tl.r0 == next_row);                        // gap-free, no overlap
    }
    CHECK(tl.r1 == hi || tl.r1 - tl.r0 == T);          // only the last is short
    next_row = tl.r1;
    rows += (uint64_t)(tl.r1 - tl.r0);
  }
  if (prev_seg >= 0) CHECK(next_row == SegHi(bounds.data(), prev_seg));
  for (int k = prev_seg + 1; k < nseg; ++k)
    CHECK(SegRows(SegLo(bounds.data(), k), SegHi(bounds.data(), k)) == 0);
  CHECK(rows == want_rows);                            // every row exactly once
  return 0;
}

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  g_seed ^= g_seed >> 12;
  g_seed ^= g_seed << 25;
  g_seed ^= g_seed >> 27;
  return g_seed * 0x2545F4914F6CDD1Dull;
}

static int check_exhaustive() {
  const int64_t B = 5;  // bounds in [0, B]
  for (int64_t T = 1; T <= 4; ++T) {
    // one query: all (B + 1)^4 bound tuples
    for (int64_t a = 0; a <= B; ++a)
      for (int64_t b = 0; b <= B; ++b)
        for (int64_t c = 0; c <= B; ++c)
          for (int64_t d = 0; d <= B; ++d)
            if (check_case({a, b, c, d}, T, B)) return 1;
    // two queries: bounds in [0, 3], all 4^8 tuples
    for (int v = 0; v < 65536; ++v) {
      std::vector<int64_t> bd(8);
      for (int k = 0; k < 8; ++k) bd[(size_t)k] = (v >> (2 * k)) & 3;
      if (check_case(bd, T, 3)) return 1;
    }
  }
  return 0;
}

static int check_tile_edges() {
  for (int64_t T : {64ll, 128ll, 4096ll}) {
    const int64_t lens[] = {0, 1, T - 1, T, T + 1, 2 * T, 2 * T + 1, 5 * T - 1};
    for (int64_t la : lens)
      for (int64_t lb : lens)
        for (int64_t off : {0ll, 1ll, 63ll, 64ll, 1000003ll}) {
          if (check_case({off, off + la, 7, 7 + lb}, T, 1ll << 40)) return 1;
          // inverted base bounds next to a real delta segment, and reverse
          if (check_case({off + la + 1, off, 0, lb}, T, 1ll << 40)) return 1;
          if (check_case({off, off + la, lb + 3, 3}, T, 1ll << 40)) return 1;
        }
  }
  return 0;
}

static int check_random() {
  const int nqs[] = {1, 2, 3, 17, 256, 1024};
  for (int it = 0; it < 240; ++it) {
    const int nq = nqs[it % 6];
    const int64_t T = ClampTile((int64_t)(64 << (rnd() % 8)));
    // regimes: mixed, mostly empty, mostly inverted, long segments
    const int regime = (it / 6) % 4;
    const int64_t n = regime == 3 ? 300000 : 5000;
    std::vector<int64_t> bd((size_t)nq * 4);
    for (int s = 0; s < 2 * nq; ++s) {
      int64_t lo = (int64_t)(rnd() % (uint64_t)(n + 1));
      int64_t hi = (int64_t)(rnd() % (uint64_t)(n + 1));
      const uint64_t r = rnd() % 8;
      if (regime == 0 && lo > hi && r) { int64_t t = lo; lo = hi; hi = t; }
      if (regime == 1 && r) hi = lo;
      if (regime == 2 && lo < hi && r) { int64_t t = lo; lo = hi; hi = t; }
      if (regime == 3 && lo > hi) { int64_t t = lo; lo = hi; hi = t; }
      bd[(size_t)(s >> 1) * 4 + (size_t)(s & 1) * 2] = lo;
      bd[(size_t)(s >> 1) * 4 + (size_t)(s & 1) * 2 + 1] = hi;
    }
    if (check_case(bd, T, n)) {
      fprintf(stderr, "random case %d (nq=%d T=%lld regime=%d) failed\n", it,
              nq, (long long)T, regime);
      return 1;
    }
  }
  return 0;
}

int main() {
  CHECK(ClampTile(0) == 64 && ClampTile(-5) == 64 && ClampTile(64) == 64);
  CHECK(ClampTile(127) == 64 && ClampTile(128) == 128 && ClampTile(4100) == 4096);
  CHECK(ClampTile(1ll << 40) == kMaxTile && kDefaultTile == ClampTile(kDefaultTile));
  if (check_exhaustive()) return 1;
  const int64_t exhaustive = g_cases;
  CHECK(exhaustive > 100000);
  if (check_tile_edges()) return 1;
  const int64_t edges = g_cases - exhaustive;
  if (check_random()) return 1;
  printf("cplan hostcheck OK (%lld exhaustive + %lld tile-edge + %lld random cases)\n",
         (long long)exhaustive, (long long)edges,
         (long long)(g_cases - exhaustive - edges));
  return 0;
}
