// kubebrain_amd/csrc/wreg.h — pure arithmetic of the batched watch
// registration (kb_watch_batch; slab.hip k_wreg_scan /
// k_wreg_plan / k_wreg_emit). The scan tests every watcher against ONE global
// grid of 64-event chunks anchored at the oldest resident ring sequence S:
// global word g, bit b = event S + 64 g + b. kb_watch instead numbers a
// watcher's catch-up bits from its OWN first sequence lo (the first ring
// event with revision >= the requested one): own word i, bit b = event
// lo + 64 i + b, and its refs cover 512 own bits each, base = lo + 512 c.
// The functions here map one numbering onto the other: own word i is a
// 64-bit funnel of the global words g0 + i and g0 + i + 1. Host and device
// share them, so wreg_hostcheck.cc proves the mapping on the CPU against the
// per-event construction kb_watch uses.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define KBW_HD __host__ __device__
#else
#define KBW_HD
#endif

namespace kbwreg {

constexpr int64_t kRefEvents = 512;   // events per pending ref (8 words)
constexpr int64_t kMinSubBatch = 64;  // one watcher slice of the scan
constexpr int64_t kDefaultBytes = 64ll << 20;  // KB_WATCH_REG_BYTES

// words of the global grid for a ring span of n events
KBW_HD inline int64_t GWords(int64_t n) { return n > 0 ? (n + 63) >> 6 : 0; }

// watchers per sub-batch: the dense scratch [watcher][gword] stays within
// `bytes`, but a sub-batch never falls below one 64-watcher slice
KBW_HD inline int64_t SubBatch(int64_t bytes, int64_t gwords) {
  const int64_t per = bytes / (8 * (gwords > 0 ? gwords : 1));
  return per < kMinSubBatch ? kMinSubBatch : per;
}

// position of a watcher's first sequence lo (S <= lo) on the global grid
KBW_HD inline int64_t G0(int64_t lo, int64_t S) { return (lo - S) >> 6; }
KBW_HD inline int Shift(int64_t lo, int64_t S) { return (int)((lo - S) & 63); }

// own word = bits [sh, sh + 64) of the 128-bit value {b : a}
KBW_HD inline uint64_t Funnel(uint64_t a, uint64_t b, int sh) {
  return sh ? (a >> sh) | (b << (64 - sh)) : a;
}

// own word i of a watcher from the global words G[0, gwords); words past the
// grid read as 0 (no event there)
KBW_HD inline uint64_t OwnWord(const uint64_t* G, int64_t gwords, int64_t g0,
                               int sh, int64_t i) {
  const int64_t g = g0 + i;
  const uint64_t a = g < gwords ? G[g] : 0;
  const uint64_t b = (sh && g + 1 < gwords) ? G[g + 1] : 0;
  return Funnel(a, b, sh);
}

// own words / refs that cnt = E - lo events can fill
KBW_HD inline int64_t OwnWords(int64_t cnt) { return cnt > 0 ? (cnt + 63) >> 6 : 0; }
KBW_HD inline int64_t MaxRefs(int64_t cnt) {
  return cnt > 0 ? (cnt + kRefEvents - 1) / kRefEvents : 0;
}
// events ref c covers: min(512, cnt - 512 c)
KBW_HD inline int32_t RefCount(int64_t cnt, int64_t c) {
  const int64_t left = cnt - kRefEvents * c;
  return (int32_t)(left < kRefEvents ? left : kRefEvents);
}
// word k of a ref with `count` events: bits at and past count are clear
KBW_HD inline uint64_t MaskWord(uint64_t w, int k, int32_t count) {
  const int32_t left = count - 64 * k;
  if (left <= 0) return 0;
  return left >= 64 ? w : w & ((1ull << left) - 1);
}

// bit l of m = own word 64 it + l is non-zero; a ref is eight consecutive own
// words, i.e. one byte of m: the non-empty refs among the eight of m
KBW_HD inline int NonEmptyRefs(uint64_t m) {
  // fold every byte onto its low bit
  m |= m >> 4;
  m |= m >> 2;
  m |= m >> 1;
  m &= 0x0101010101010101ull;
  return (int)((m * 0x0101010101010101ull) >> 56);
}
// non-empty refs of m below ref r (r in [0, 8])
KBW_HD inline int NonEmptyRefsBelow(uint64_t m, int r) {
  return r >= 8 ? NonEmptyRefs(m) : NonEmptyRefs(m & ((1ull << (8 * r)) - 1));
}

struct Ref {  // == kbslab::WpollRef
  int64_t base;
  int32_t count;
  int32_t widx;
  uint64_t words[8];
};
static_assert(sizeof(Ref) == 80, "ref layout");

// host form of k_wreg_plan + k_wreg_emit for one watcher: the non-empty refs
// of the ring span [lo, E) in ascending order. out has room for MaxRefs(E -
// lo) entries (may be null to count only); *pend = events queued.
inline int64_t BuildRefs(const uint64_t* G, int64_t gwords, int64_t S,
                         int64_t lo, int64_t E, int32_t widx, Ref* out,
                         int64_t* pend) {
  const int64_t cnt = E - lo, g0 = G0(lo, S);
  const int sh = Shift(lo, S);
  int64_t n = 0, total = 0;
  for (int64_t c = 0; c < MaxRefs(cnt); ++c) {
    Ref r{};
    r.base = lo + kRefEvents * c;
    r.count = RefCount(cnt, c);
    r.widx = widx;
    int64_t got = 0;
    for (int k = 0; k < 8; ++k) {
      r.words[k] = MaskWord(OwnWord(G, gwords, g0, sh, 8 * c + k), k, r.count);
      got += __builtin_popcountll(r.words[k]);
    }
    if (!got) continue;
    if (out) out[n] = r;
    ++n;
    total += got;
  }
  if (pend) *pend = total;
  return n;
}

}  // namespace kbwreg
