// kubebrain_amd/csrc/cplan.h — tile map of the batched Count (kb_count_batch,
// DESIGN.md §3.8; slab.hip k_count_plan / k_count_tiles). A launch of nq
// queries has 2 * nq row segments, interleaved per query: the base run's
// [lo, hi) then the delta run's [dlo, dhi) — the four values k_range_bounds
// writes per query. Every segment is cut into tiles of T rows; an exclusive
// prefix over the segments' tile counts numbers the tiles of the launch, and
// a tile id maps back to {query, run, r0, r1} by binary search over it.
// Host and device share these functions, so cplan_hostcheck.cc proves the
// map against naive enumeration on the CPU.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define KBC_HD __host__ __device__
#else
#define KBC_HD
#endif

namespace kbcount {

constexpr int64_t kMinTile = 64;           // one wave slice
constexpr int64_t kMaxTile = 1ll << 20;
constexpr int64_t kDefaultTile = 4096;

// KB_COUNT_TILE as a store takes it: a multiple of 64 in [kMinTile, kMaxTile]
KBC_HD inline int64_t ClampTile(int64_t t) {
  if (t < kMinTile) return kMinTile;
  if (t > kMaxTile) return kMaxTile;
  return t & ~63ll;
}

// rows of segment [lo, hi); inverted bounds (start >= end) hold none
KBC_HD inline int64_t SegRows(int64_t lo, int64_t hi) {
  return hi > lo ? hi - lo : 0;
}

// tiles of segment [lo, hi): max(0, hi - lo + T - 1) / T
KBC_HD inline uint64_t SegTiles(int64_t lo, int64_t hi, int64_t T) {
  return hi > lo ? (uint64_t)((hi - lo + T - 1) / T) : 0;
}

// bounds of segment s in the per-query {lo, hi, dlo, dhi} table
KBC_HD inline int64_t SegLo(const int64_t* bounds, int s) {
  return bounds[(int64_t)(s >> 1) * 4 + (s & 1) * 2];
}
KBC_HD inline int64_t SegHi(const int64_t* bounds, int s) {
  return bounds[(int64_t)(s >> 1) * 4 + (s & 1) * 2 + 1];
}

// the segment that holds tile t: the s with pfx[s] <= t < pfx[s + 1], for
// t < pfx[nseg]. Segments without tiles are never returned (pfx[s] ==
// pfx[s + 1] cannot straddle t).
KBC_HD inline int FindSeg(const uint64_t* pfx, int nseg, uint64_t t) {
  int lo = 0, hi = nseg;  // first s in [0, nseg] with pfx[s] > t, minus one
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (pfx[mid + 1] <= t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct Tile {
  int32_t query, run;  // run 0 = base, 1 = delta
  int64_t r0, r1;      // rows [r0, r1) of that run, r1 = min(r0 + T, hi)
  int64_t hi;          // end of the SEGMENT (guards the rev[i + 1] load)
};

KBC_HD inline Tile MapTile(const int64_t* bounds, const uint64_t* pfx, int nseg,
                           uint64_t t, int64_t T) {
  const int s = FindSeg(pfx, nseg, t);
  const int64_t lo = SegLo(bounds, s), hi = SegHi(bounds, s);
  Tile o;
  o.query = s >> 1;
  o.run = s & 1;
  o.r0 = lo + (int64_t)(t - pfx[s]) * T;
  o.r1 = o.r0 + T < hi ? o.r0 + T : hi;
  o.hi = hi;
  return o;
}

// host form of k_count_plan: pfx[0 .. 2 * nq], returns the tile total
inline uint64_t BuildPrefix(const int64_t* bounds, int nq, int64_t T,
                            uint64_t* pfx) {
  uint64_t acc = 0;
  for (int s = 0; s < 2 * nq; ++s) {
    pfx[s] = acc;
    acc += SegTiles(SegLo(bounds, s), SegHi(bounds, s), T);
  }
  pfx[2 * nq] = acc;
  return acc;
}

}  // namespace kbcount
