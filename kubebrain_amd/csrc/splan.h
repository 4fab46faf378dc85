// kubebrain_amd/csrc/splan.h — window, tile and cut arithmetic of the batched
// stream read (kb_stream_next_batch; slab.hip k_stream_*).
// A call scans the rest of a stream's range window by window. A window is the
// base rows [lo, e) with e = min(lo + W, hi) plus the delta rows [dlo, dhiw):
// when the window stops short of the base bound, the delta segment stops at
// the first delta row of the key of base row e, so every winner of this window
// sorts before every winner of the next. Both segments are cut into tiles of
// kTile rows (16 slices of 64 rows, one ballot word each, numbered from the
// segment's first row). The merged winners' wire sizes are then cut to the
// largest n that respects max_kvs, the caller's buffer and the arena.
// Host and device share these functions, so splan_hostcheck.cc proves them
// against naive loops on the CPU.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define KBS_HD __host__ __device__
#else
#define KBS_HD
#endif

namespace kbstream {

constexpr int64_t kMinWindow = 64;            // one wave slice
constexpr int64_t kMaxWindow = 1ll << 26;
constexpr int64_t kDefaultWindow = 1ll << 18;
constexpr int64_t kTile = 1024;               // rows per mark tile
constexpr int64_t kDefaultMaxKvs = 65536;     // KB_STREAM_MAX_KVS
constexpr int64_t kMaxMaxKvs = 1ll << 24;

// KB_STREAM_WINDOW as a store takes it: a multiple of 64 in [kMinWindow,
// kMaxWindow], clamped the way KB_COUNT_TILE is
KBS_HD inline int64_t ClampWindow(int64_t w) {
  if (w < kMinWindow) return kMinWindow;
  if (w > kMaxWindow) return kMaxWindow;
  return w & ~63ll;
}

KBS_HD inline int64_t ClampMaxKvs(int64_t m) {
  if (m < 1) return kDefaultMaxKvs;
  return m > kMaxMaxKvs ? kMaxMaxKvs : m;
}

// records one call may return: max_kvs <= 0 or above the library's maximum
// means that maximum
KBS_HD inline int64_t ResolveMaxKvs(int64_t req, int64_t lib_max) {
  return (req <= 0 || req > lib_max) ? lib_max : req;
}

// a bound pair as the kernels use it: 0 <= lo <= hi <= n (inverted bounds
// hold no row)
KBS_HD inline int64_t ClampLo(int64_t lo, int64_t n) {
  return lo < 0 ? 0 : (lo > n ? n : lo);
}
KBS_HD inline int64_t ClampHi(int64_t lo, int64_t hi, int64_t n) {
  if (hi > n) hi = n;
  return hi < lo ? lo : hi;
}

// end of the window over base rows [lo, hi): at most W rows
KBS_HD inline int64_t WindowEnd(int64_t lo, int64_t hi, int64_t W) {
  if (hi <= lo) return lo;
  return hi - lo > W ? lo + W : hi;
}

// the delta end rule. A window that reaches the base bound (e >= hi) takes
// the whole rest [dlo, dhi) of the delta segment; one that stops at base row
// e < hi takes the delta rows below key_lb = lower bound of (key(e), rev 0)
// in the delta run, held inside [dlo, dhi].
KBS_HD inline int64_t DeltaEnd(int64_t e, int64_t hi, int64_t dlo, int64_t dhi,
                               int64_t key_lb) {
  if (dhi < dlo) dhi = dlo;
  if (e >= hi) return dhi;
  if (key_lb < dlo) return dlo;
  return key_lb > dhi ? dhi : key_lb;
}

KBS_HD inline int64_t SegWords(int64_t rows) { return rows > 0 ? (rows + 63) >> 6 : 0; }
KBS_HD inline uint64_t SegTiles(int64_t rows) {
  return rows > 0 ? (uint64_t)((rows + kTile - 1) / kTile) : 0;
}

struct Tile {
  int32_t run;     // 0 = base, 1 = delta
  int64_t r0, r1;  // rows [r0, r1) of that run; r0 - segment start is a
                   // multiple of kTile, so its slices are whole ballot words
};

// tile t of a window: the base segment's tiles first, then the delta's
KBS_HD inline Tile MapTile(int64_t lo, int64_t e, int64_t dlo, int64_t dhiw,
                           uint64_t t) {
  const uint64_t nb = SegTiles(e - lo);
  Tile o;
  o.run = t >= nb;
  const int64_t s0 = o.run ? dlo : lo, s1 = o.run ? dhiw : e;
  o.r0 = s0 + (int64_t)(o.run ? t - nb : t) * kTile;
  o.r1 = o.r0 + kTile < s1 ? o.r0 + kTile : s1;
  return o;
}

// wire bytes of one record: u64 rev; u32 klen; key; u32 vlen; val
KBS_HD inline uint64_t RecordBytes(uint32_t klen, uint32_t vlen) {
  return 16 + (uint64_t)klen + vlen;
}

// byte budget of the records of one reply: the caller's buffer minus the u32
// count, and never more than one arena holds
KBS_HD inline uint64_t CutLimit(uint64_t cap, uint64_t arena) {
  if (cap < 4) return 0;
  return cap - 4 < arena ? cap - 4 : arena;
}

// does merged record j, at exclusive byte offset off with sz wire bytes, fall
// inside the cut? off + sz grows with j, so the records that fit form a
// prefix and their number is the cut.
KBS_HD inline bool Fits(uint64_t j, uint64_t off, uint64_t sz, uint64_t max_kvs,
                        uint64_t lim) {
  return j < max_kvs && sz <= lim && off <= lim - sz;
}

// KB_ENOBUF: what the caller's buffer has to hold for the next record alone
KBS_HD inline uint64_t EnobufSize(uint64_t first_size) { return 4 + first_size; }

// host form of k_stream_cut: the largest n under the three bounds
struct Cut { uint64_t n, bytes; };
inline Cut CutTable(const uint64_t* sizes, uint64_t ntab, uint64_t max_kvs,
                    uint64_t lim) {
  Cut c{0, 0};
  for (uint64_t j = 0; j < ntab; ++j) {
    if (!Fits(j, c.bytes, sizes[j], max_kvs, lim)) break;
    c.bytes += sizes[j];
    c.n = j + 1;
  }
  return c;
}

}  // namespace kbstream
