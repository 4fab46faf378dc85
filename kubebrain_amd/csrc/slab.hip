// kubebrain_amd/csrc/slab.hip — MI355X (gfx950) HBM slab engine.
//
// All device kernels of the MVCC hot path. HBM-bound
// integer/byte work by design (north_star: indexing/scan, no MFMA):
// wavefront = 64 lanes, __ballot is 64-bit, coalesced 16B-per-lane loads
// where layout permits. Semantics cites are into /root/reference.

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstring>

#include "cplan.h"
#include "dmerge.h"
#include "slab_dev.h"
#include "stepstage.h"

namespace kbslab {

#define HIP_CHECK(expr)                                                    \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess) {                                                \
      if (err) *err = std::string(#expr) + ": " + hipGetErrorString(_e);   \
      return false;                                                        \
    }                                                                      \
  } while (0)

#define HIP_CHECK_NULL(expr)                                               \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess) {                                                \
      if (err) *err = std::string(#expr) + ": " + hipGetErrorString(_e);   \
      return nullptr;                                                      \
    }                                                                      \
  } while (0)

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------- device ---

// byte-lexicographic compare of two 96B zero-padded keys (== internal-key
// order for keys with bytes > '$'; coder/normal.go:29-31).
__device__ __forceinline__ int keycmp96(const uint8_t* a, const uint8_t* b) {
  const uint64_t* A = (const uint64_t*)a;
  const uint64_t* B = (const uint64_t*)b;
#pragma unroll
  for (int i = 0; i < KEYW / 8; ++i) {
    uint64_t x = A[i], y = B[i];
    if (x != y) {
      x = __builtin_bswap64(x);
      y = __builtin_bswap64(y);
      return x < y ? -1 : 1;
    }
  }
  return 0;
}

// Full-key compare with spill tails (keys > KEYW): the 96B
// zero-padded prefix decides every compare except exact 96-byte prefix ties
// — only possible when BOTH keys are >= 96B (key bytes are > 0x24 > 0x00) —
// which compare their tails from the spill heaps. The tail loop runs on the
// rare tie path only; the hot predicate never touches it.
__device__ __forceinline__ int keycmp_ext(
    const uint8_t* a96, uint32_t alen, uint64_t ako, const uint8_t* aspill,
    const uint8_t* b96, uint32_t blen, uint64_t bko, const uint8_t* bspill) {
  int c = keycmp96(a96, b96);
  if (c || (alen <= (uint32_t)KEYW && blen <= (uint32_t)KEYW)) return c;
  uint32_t at = alen > (uint32_t)KEYW ? alen - KEYW : 0;
  uint32_t bt = blen > (uint32_t)KEYW ? blen - KEYW : 0;
  const uint8_t* ap = aspill + ako;
  const uint8_t* bp = bspill + bko;
  uint32_t m = at < bt ? at : bt;
  for (uint32_t i = 0; i < m; ++i)
    if (ap[i] != bp[i]) return ap[i] < bp[i] ? -1 : 1;
  return at == bt ? 0 : (at < bt ? -1 : 1);
}

// one sorted run's columns (base or delta); spill is shared store-wide
struct Run {
  const uint8_t* keys;
  const uint64_t* meta;
  const uint64_t* rev;
  const uint64_t* vo;
  const uint64_t* ko;
};

// a query-side key: 96B padded prefix + optional tail in `tails`
struct QKey {
  const uint8_t* k96;
  uint32_t len;
  uint64_t ko;
  const uint8_t* tails;
};

__device__ __forceinline__ QKey row_qk(const Run& r, const uint8_t* spill,
                                       int64_t i) {
  return QKey{r.keys + i * KEYW, meta_klen(r.meta[i]), r.ko[i], spill};
}

__device__ __forceinline__ int rowcmp_q(const Run& r, const uint8_t* spill,
                                        int64_t i, const QKey& q) {
  return keycmp_ext(r.keys + i * KEYW, meta_klen(r.meta[i]), r.ko[i], spill,
                    q.k96, q.len, q.ko, q.tails);
}

// first row in [lo,hi) with (key,rev) >= (q,qrev)
__device__ int64_t d_lb_range(const Run& r, const uint8_t* spill, int64_t lo,
                              int64_t hi, const QKey& q, uint64_t qrev) {
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    int c = rowcmp_q(r, spill, mid, q);
    if (c < 0 || (c == 0 && r.rev[mid] < qrev)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// wave-cooperative 64-ary lower bound: every round all 64 lanes probe one
// pivot each (64 independent loads in ONE memory round trip), the ballot of
// "pivot < q" collapses the range 64x. Depth log64(n): a 21M-row slab costs
// ~5 round trips where the serial binary search pays ~25 dependent ones.
// All lanes of the wave must call; the result is wave-uniform.
__device__ int64_t d_lb_wave(const Run& r, const uint8_t* spill, int64_t n,
                             const QKey& q, uint64_t qrev) {
  const int lane = threadIdx.x & 63;
  int64_t lo = 0, hi = n;  // answer in [lo, hi]
  while (hi - lo > 64) {
    int64_t step = (hi - lo) >> 6;  // >= 1
    int64_t p = lo + (int64_t)(lane + 1) * step;
    bool lt = false;  // keys[p] < q (monotone non-increasing in p)
    if (p < hi) {
      int c = rowcmp_q(r, spill, p, q);
      lt = c < 0 || (c == 0 && r.rev[p] < qrev);
    }
    int k = __popcll(__ballot(lt));
    int64_t nlo = lo + (int64_t)k * step;
    int64_t nhi = k == 64 ? hi : min(lo + (int64_t)(k + 1) * step, hi);
    lo = nlo;
    hi = nhi;
  }
  int64_t p = lo + lane;
  bool ge = false;  // first in-range row with keys[p] >= q
  if (p < hi) {
    int c = rowcmp_q(r, spill, p, q);
    ge = !(c < 0 || (c == 0 && r.rev[p] < qrev));
  }
  uint64_t b = __ballot(ge);
  return b ? lo + (__ffsll((unsigned long long)b) - 1) : hi;
}

// block-wide exclusive scan of one value per thread: shuffles inside each
// wave, one LDS hop (wsum[blockDim.x / 64]) across waves, two barriers. Every
// thread of the block must call; blockDim.x is a multiple of 64. *total =
// the block's sum, in every thread. wsum may be reused after the call.
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* wsum, T* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nw = blockDim.x >> 6;
  T inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    T o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  T base = 0, tot = 0;
  for (int i = 0; i < nw; ++i) {
    T s = wsum[i];
    if (i < w) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// adjacent-row full-key equality (same spill both sides)
__device__ __forceinline__ bool rows_same_key(const uint8_t* keys,
                                              const uint64_t* meta,
                                              const uint64_t* ko,
                                              const uint8_t* spill, int64_t i,
                                              int64_t j) {
  const uint64_t* a = (const uint64_t*)(keys + i * KEYW);
  const uint64_t* b = (const uint64_t*)(keys + j * KEYW);
#pragma unroll
  for (int k = 0; k < KEYW / 8; ++k)
    if (a[k] != b[k]) return false;
  uint32_t al = meta_klen(meta[i]), bl = meta_klen(meta[j]);
  if (al <= (uint32_t)KEYW && bl <= (uint32_t)KEYW) return true;
  if (al != bl) return false;
  const uint8_t* ap = spill + ko[i];
  const uint8_t* bp = spill + ko[j];
  for (uint32_t t = 0; t < al - (uint32_t)KEYW; ++t)
    if (ap[t] != bp[t]) return false;
  return true;
}

// ---- same_next: adjacent-key equality bits over one run ----
__global__ void k_same_next(const uint8_t* __restrict__ keys,
                            uint64_t* __restrict__ meta,
                            const uint64_t* __restrict__ ko,
                            const uint8_t* __restrict__ spill, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t m = meta[i];
  bool same = i + 1 < n && rows_same_key(keys, meta, ko, spill, i, i + 1);
  meta[i] = same ? (m | M_SAME_NEXT) : (m & ~M_SAME_NEXT);
}

constexpr uint64_t ROW_TAG_DELTA = 1ull << 63;  // winner row lives in the delta run
constexpr uint64_t ROW_MASK = ROW_TAG_DELTA - 1;

// ---- two-run variant: base run + sorted delta run merged at scan time ---
// The delta run holds rows strictly newer than the base run's rows of the
// same key, so the global winner of a key is the delta
// winner when the delta has any row of the key with rev<=R, else the base
// winner — base winners are suppressed by a delta probe, and the two ordered
// winner lists are merged by rank (keys never collide across lists).

// scan block width: runtime-tunable (KB_SCAN_T in {256,512,1024}); the
// kernel reads blockDim.x, only the LDS wave-count array is sized for the max
constexpr int SCAN_T_MAX = 1024;

// shadow-revision column (base run only): shadow[i] = smallest delta-run
// revision (>=1) of base row i's key, UINT64_MAX = the delta holds no row of
// that key. Maintained by k_shadow_mark at delta-insert time and reset to
// MAX whenever the base is rebuilt (fold/compact empty the delta). Turns the
// scan's winner-suppression probe — a per-winner binary search over the
// delta — into one coalesced 8B stream read: base winner i is suppressed
// iff shadow[i] != MAX && shadow[i] <= R (a strictly-newer delta row of the
// key exists at or below the read revision).
//
// One wave per uploaded row (4 per 256-thread block): the 64-ary wave search
// finds the key's first base row in ~5 round trips, one key compare confirms
// it, and the key's run is then walked by its M_SAME_NEXT bits alone — 256
// rows per round trip (four independent meta loads per lane), no key bytes.
__global__ __launch_bounds__(256) void k_shadow_mark(
    Run b, int64_t n, Run dnew, int64_t m, const uint8_t* __restrict__ spill,
    uint64_t* __restrict__ shadow) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= m) return;  // wave-uniform from here on
  const uint64_t rv = dnew.rev[j];
  if (rv == 0) return;  // rev-row holes never suppress
  QKey k = row_qk(dnew, spill, j);
  const int64_t lb = d_lb_wave(b, spill, n, k, 1);
  if (lb >= n || rowcmp_q(b, spill, lb, k) != 0) return;  // no base row
  for (int64_t c = lb; c < n; c += 256) {
    uint64_t mm[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = c + u * 64 + lane;
      mm[u] = i < n ? b.meta[i] : 0;  // 0: the run ends at or before row n-1
    }
    bool done = false;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (done) break;
      const int64_t i = c + u * 64 + lane;
      // lanes whose row is not followed by another row of the key; the first
      // of them holds the run's last row (or lies past the run's end at n)
      const uint64_t ends = __ballot(!(mm[u] & M_SAME_NEXT));
      const int last = ends ? __ffsll((unsigned long long)ends) - 1 : 64;
      if (lane <= last && i < n)
        atomicMin((unsigned long long*)&shadow[i], (unsigned long long)rv);
      done = ends != 0;
    }
    if (done) break;
  }
}

// one run's winner scan (ordered append); returns written, *total = seen.
// Two-pass per tile: (1) each wave reads a CONTIGUOUS chunk of rows with
// fully-coalesced 8B meta/rev streams, recording winner flags in a register
// bitmask -- no LDS, no syncs inside the pass; (2) after one barrier
// publishes the per-wave totals, a register-only ballot replay scatters the
// winner row indices at their ordered offsets. Two __syncthreads per tile
// of up to NW*4096 rows (the old design paid two per 1024 rows).
__device__ int64_t scan_run_winners(
    const Run& run, const uint8_t* spill, int64_t lo, int64_t hi, uint64_t R,
    int64_t cap, uint64_t* out, int64_t out_cap, uint64_t tagbit,
    const uint64_t* shadow,  // shadow-revision column (null => no suppression)
    int64_t* total_out, int64_t* scanned_accum, int* wave_cnt,
    unsigned long long* dbg) {  // KB_SCAN_DBG phase cycles (null in prod)
  const uint64_t* __restrict__ rev = run.rev;
  const uint64_t* __restrict__ meta = run.meta;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int NW = blockDim.x >> 6;
  const int64_t span = hi - lo;
  if (span <= 0) { *total_out = 0; return 0; }
  // per-wave chunk: cover the span in one tile when it fits (<= NW*4096
  // rows); for capped queries over much larger spans, tile by a winner-
  // density heuristic so the cap early-exit still bounds the read volume
  int64_t target = span;
  if (cap != INT64_MAX && 6 * cap < span) target = 6 * cap;
  int64_t C = (target + NW - 1) / NW;
  C = (C + 63) & ~63ll;
  if (C > 4096) C = 4096;
  const int64_t TILE = (int64_t)NW * C;
  int64_t scanned = 0;
  int64_t cnt = 0;  // winners before this tile (uniform across the block)
  const bool dbg0 = dbg && threadIdx.x == 0;
  unsigned long long tprev = dbg0 ? wall_clock64() : 0;
  for (int64_t t = lo; t < hi; t += TILE) {
    const int64_t wbase = t + (int64_t)w * C;
    int rounds = 0;
    if (wbase < hi) rounds = (int)((min(C, hi - wbase) + 63) >> 6);
    // pass 1a: streaming winner predicate — rev/meta 8B streams only, no
    // probes and no divergent chains, so the loads pipeline across rounds.
    // same_next set => row i+1 exists, shares the key, and (rows of one key
    // being contiguous and its key < qend) lies below hi, so the rev[i+1]
    // load is gated by i+1<hi alone, independent of the meta bits.
    // pass 1: streaming winner predicate — rev/meta/shadow 8B streams only,
    // no probes and no divergent chains, so the loads pipeline across
    // rounds. same_next set => row i+1 exists, shares the key, and (rows of
    // one key being contiguous and its key < qend) lies below hi, so the
    // rev[i+1] load is gated by i+1<hi alone, independent of the meta bits.
    // Suppression is the shadow-revision stream: a base winner loses iff a
    // strictly-newer delta row of its key exists at or below R.
    uint64_t flags = 0;
    // full rounds carry no bounds check (every lane in range), so the
    // rev/meta/shadow loads have no control dependence and pipeline across
    // the unrolled iterations; only the ragged tail round is guarded
    const int full = (int)min((int64_t)rounds, (hi - wbase) >> 6);
#pragma unroll 4
    for (int r = 0; r < full; ++r) {
      int64_t i = wbase + ((int64_t)r << 6) + lane;
      uint64_t rv = rev[i], m = meta[i];
      uint64_t rvn = (i + 1 < hi) ? rev[i + 1] : 0;
      uint64_t sh = shadow ? shadow[i] : UINT64_MAX;
      bool win = false;
      if (rv > 0 && rv <= R && !(m & M_TOMB) &&
          !(sh != UINT64_MAX && sh <= R))
        win = !(m & M_SAME_NEXT) || rvn > R;
      if (win) flags |= 1ull << r;
    }
    for (int r = full; r < rounds; ++r) {
      int64_t i = wbase + ((int64_t)r << 6) + lane;
      bool win = false;
      if (i < hi) {
        uint64_t rv = rev[i], m = meta[i];
        uint64_t rvn = (i + 1 < hi) ? rev[i + 1] : 0;
        uint64_t sh = shadow ? shadow[i] : UINT64_MAX;
        if (rv > 0 && rv <= R && !(m & M_TOMB) &&
            !(sh != UINT64_MAX && sh <= R))
          win = !(m & M_SAME_NEXT) || rvn > R;
      }
      if (win) flags |= 1ull << r;
    }
    if (dbg0) { unsigned long long t1 = wall_clock64(); atomicAdd(&dbg[1], t1 - tprev); tprev = t1; }
    uint32_t wcnt = 0;
    for (int r = 0; r < rounds; ++r)
      wcnt += (uint32_t)__popcll(__ballot((flags >> r) & 1));
    if (dbg0) { unsigned long long t2 = wall_clock64(); atomicAdd(&dbg[2], t2 - tprev); tprev = t2; }
    if (lane == 0) wave_cnt[w] = (int)wcnt;
    __syncthreads();
    int64_t waveoff = 0, tile_total = 0;
    for (int k = 0; k < NW; ++k) {
      if (k < w) waveoff += wave_cnt[k];
      tile_total += wave_cnt[k];
    }
    // pass 2: ordered scatter by ballot replay (no memory re-reads)
    if (out && wcnt) {
      uint32_t done = 0;
      for (int r = 0; r < rounds; ++r) {
        uint64_t b = __ballot((flags >> r) & 1);
        if ((flags >> r) & 1) {
          int64_t idx = cnt + waveoff + done +
                        (int64_t)__popcll(b & ((1ull << lane) - 1));
          if (idx < cap && idx < out_cap)
            out[idx] = (uint64_t)(wbase + ((int64_t)r << 6) + lane) | tagbit;
        }
        done += (uint32_t)__popcll(b);
      }
    }
    if (dbg0) { unsigned long long t3 = wall_clock64(); atomicAdd(&dbg[3], t3 - tprev); tprev = t3; }
    cnt += tile_total;
    scanned += min(TILE, hi - t);
    if (cnt >= cap) break;
    __syncthreads();  // wave_cnt reused next tile
  }
  *total_out = cnt;
  if (scanned_accum) *scanned_accum += scanned;
  int64_t written = cnt < cap ? cnt : cap;
  if (written > out_cap) written = out_cap;
  return out ? written : 0;
}

// lower_bound over a winner list via key indirection (no cross-list ties)
__device__ int64_t d_lb_winlist(const uint64_t* rows, int64_t n, const Run& b,
                                const Run& d, const uint8_t* spill,
                                const QKey& q) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    uint64_t rt = rows[mid];
    const Run& rr = (rt & ROW_TAG_DELTA) ? d : b;
    if (rowcmp_q(rr, spill, (int64_t)(rt & ROW_MASK), q) < 0) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// bounds pre-pass: one 256-thread block per query, its 4 waves resolving the
// 4 run bounds concurrently via the wave-cooperative 64-ary search. As a
// standalone launch all 4*nq searches overlap chip-wide; inside the scan
// kernel they sat on every block's critical path (~7 us serial per block).
__global__ void k_range_bounds(Run b, int64_t n, Run d, int64_t dn,
                               const uint8_t* __restrict__ spill,
                               const uint8_t* __restrict__ qtails,
                               const DevRangeQ* __restrict__ qs, int nq,
                               int64_t* __restrict__ bounds_g /*[4*nq]*/,
                               unsigned long long* __restrict__ counters) {
  int q = blockIdx.x;
  if (q >= nq) return;
  // rows-scanned / bytes-gathered of this batch start at 0: the scan and the
  // gather that add to them follow this kernel in stream order, and the
  // previous batch's read-back of them precedes it
  if (q == 0 && threadIdx.x == 0) { counters[0] = 0; counters[1] = 0; }
  const DevRangeQ& Q = qs[q];
  const QKey qstart{Q.start, Q.start_klen, Q.start_ko, qtails};
  const QKey qend{Q.end, Q.end_klen, Q.end_ko, qtails};
  int w = threadIdx.x >> 6;
  int64_t r = -1;
  if (w == 0) r = d_lb_wave(b, spill, n, qstart, Q.start_rev);
  else if (w == 1) r = d_lb_wave(b, spill, n, qend, 0);
  else if (w == 2) r = d_lb_wave(d, spill, dn, qstart, Q.start_rev);
  else if (w == 3) r = d_lb_wave(d, spill, dn, qend, 0);
  if (w < 4 && (threadIdx.x & 63) == 0) bounds_g[(int64_t)q * 4 + w] = r;
}

__global__ void k_range_scan2(
    Run b, int64_t n, Run d, int64_t dn, const uint8_t* __restrict__ spill,
    const uint8_t* __restrict__ qtails, const DevRangeQ* __restrict__ qs,
    int nq, int64_t max_cap,
    uint64_t* __restrict__ rows_b, uint64_t* __restrict__ rows_d,
    uint64_t* __restrict__ rows_m, int64_t* __restrict__ found_out,
    int64_t* __restrict__ total_out, unsigned long long* __restrict__ scanned_out,
    const int64_t* __restrict__ bounds_g,  // from k_range_bounds
    const uint64_t* __restrict__ shadow,  // base shadow-revision column
    unsigned long long* dbg) {  // KB_SCAN_DBG phase cycles (null in prod)
  int q = blockIdx.x;
  if (q >= nq) return;
  __shared__ int wave_cnt[SCAN_T_MAX / 64];
  const DevRangeQ& Q = qs[q];
  const bool dbg0 = dbg && threadIdx.x == 0;
  unsigned long long tk0 = dbg0 ? wall_clock64() : 0;
  // bounds resolved by the k_range_bounds pre-pass
  const int64_t lo_s = bounds_g[(int64_t)q * 4 + 0];
  const int64_t hi_s = bounds_g[(int64_t)q * 4 + 1];
  const int64_t dlo_s = bounds_g[(int64_t)q * 4 + 2];
  const int64_t dhi_s = bounds_g[(int64_t)q * 4 + 3];
  if (dbg0) { unsigned long long tkb = wall_clock64(); atomicAdd(&dbg[0], tkb - tk0); }
  const int64_t cap = Q.cap > 0 ? Q.cap : INT64_MAX;
  int64_t scanned = 0;
  int64_t dtotal = 0, btotal = 0;
  uint64_t* outd = Q.count_only ? nullptr : rows_d + (int64_t)q * max_cap;
  uint64_t* outb = Q.count_only ? nullptr : rows_b + (int64_t)q * max_cap;
  int64_t nB = scan_run_winners(d, spill, dlo_s, dhi_s, Q.read_rev,
                                cap, outd, max_cap, ROW_TAG_DELTA, nullptr,
                                &dtotal, &scanned, wave_cnt, dbg);
  __syncthreads();  // wave_cnt handoff between the two runs
  int64_t nA = scan_run_winners(b, spill, lo_s, hi_s, Q.read_rev, cap,
                                outb, max_cap, 0, dn ? shadow : nullptr,
                                &btotal, &scanned, wave_cnt, dbg);
  __syncthreads();  // winner lists complete before the merge reads them
  unsigned long long tkm = dbg0 ? wall_clock64() : 0;
  // merge by rank into rows_m (keys are disjoint across the two lists)
  int64_t cap_m = nA + nB;
  if (cap_m > cap) cap_m = cap;
  if (cap_m > max_cap) cap_m = max_cap;
  if (!Q.count_only) {
    uint64_t* outm = rows_m + (int64_t)q * max_cap;
    for (int64_t j = threadIdx.x; j < nA + nB; j += blockDim.x) {
      uint64_t rt;
      int64_t pos;
      if (j < nA) {
        rt = outb[j];
        QKey k = row_qk(b, spill, (int64_t)(rt & ROW_MASK));
        pos = j + d_lb_winlist(outd, nB, b, d, spill, k);
      } else {
        rt = outd[j - nA];
        QKey k = row_qk(d, spill, (int64_t)(rt & ROW_MASK));
        pos = (j - nA) + d_lb_winlist(outb, nA, b, d, spill, k);
      }
      if (pos < cap_m) outm[pos] = rt;
    }
  }
  if (dbg0) {
    unsigned long long tke = wall_clock64();
    atomicAdd(&dbg[4], tke - tkm);
    atomicAdd(&dbg[5], tke - tk0);
    atomicMax(&dbg[6], tke - tk0);  // slowest block (tail skew diagnostic)
    atomicAdd(&dbg[7], 1ull);
  }
  if (threadIdx.x == 0) {
    total_out[q] = btotal + dtotal;
    found_out[q] = Q.count_only ? 0 : cap_m;
    atomicAdd(scanned_out, (unsigned long long)scanned);
  }
}

// two-run point read: the delta run wins when it has any row of the key <= R
__global__ void k_get2(Run b, Run d, int64_t n, int64_t dn,
                       const uint8_t* __restrict__ spill,
                       const uint8_t* __restrict__ qtails,
                       const uint8_t* __restrict__ heap,
                       const DevGetQ* __restrict__ qs, int nq, int copy_vals,
                       uint8_t* __restrict__ out, int64_t slot,
                       uint64_t* __restrict__ orev, uint64_t* __restrict__ ometa,
                       int32_t* __restrict__ ofound, int32_t* __restrict__ oovf) {
  int q = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (q >= nq) return;
  const DevGetQ& Q = qs[q];
  const QKey qk{Q.key, Q.klen, Q.ko, qtails};
  int64_t row = -1;
  int isdelta = 0;
  // upper_bound(key,R) == lower_bound(key,R+1); R+1 saturates safely (real
  // revisions are far below UINT64_MAX). Wave-cooperative searches: the
  // whole wave runs each 64-ary probe round in one memory round trip.
  uint64_t nr = Q.read_rev == UINT64_MAX ? UINT64_MAX : Q.read_rev + 1;
  if (dn > 0) {
    int64_t ub = d_lb_wave(d, spill, dn, qk, nr);
    if (ub > 0) {
      int64_t c = ub - 1;
      if (d.rev[c] >= 1 && rowcmp_q(d, spill, c, qk) == 0) {
        row = c;
        isdelta = 1;
      }
    }
  }
  if (row < 0) {
    int64_t ub = d_lb_wave(b, spill, n, qk, nr);
    if (ub > 0) {
      int64_t c = ub - 1;
      if (b.rev[c] >= 1 && rowcmp_q(b, spill, c, qk) == 0) row = c;
    }
  }
  if (row < 0) {
    if (lane == 0) { ofound[q] = 0; oovf[q] = 0; }
    return;
  }
  const uint64_t* meta = isdelta ? d.meta : b.meta;
  const uint64_t* rev = isdelta ? d.rev : b.rev;
  const uint64_t* vo = isdelta ? d.vo : b.vo;
  uint64_t m = meta[row];
  uint32_t vlen = meta_vlen(m);
  if (lane == 0) {
    ofound[q] = 1;
    orev[q] = rev[row];
    ometa[q] = m;
    oovf[q] = (copy_vals && vlen > slot) ? 1 : 0;
  }
  if (!copy_vals || vlen > slot) return;
  const uint8_t* vs = heap + vo[row];
  uint8_t* vd = out + (int64_t)q * slot;
  uint32_t w16 = vlen >> 4;
  for (uint32_t b = lane; b < w16; b += 64)
    ((uint4*)vd)[b] = ((const uint4*)vs)[b];
  if (lane == 0)
    for (uint32_t b = w16 * 16; b < vlen; ++b) vd[b] = vs[b];
}

// ---- gather: winners -> packed records in the per-query device arena ----
// record: u64 rev | u32 klen | u32 vlen | key (pad8) | val (pad8)
__device__ __forceinline__ int64_t rec_bytes(uint32_t klen, uint32_t vlen) {
  // 16B-aligned record: header | key pad16 | value pad16 (uint4 copies)
  return 16 + ((klen + 15) & ~15u) + ((vlen + 15) & ~15u);
}

__global__ void k_gather(Run b, Run d,
                         const uint8_t* __restrict__ heap,
                         const uint64_t* __restrict__ rows_out, int64_t max_cap,
                         const int64_t* __restrict__ found_out,
                         const DevRangeQ* __restrict__ qs, int nq,
                         uint8_t* __restrict__ gbuf, int64_t qcap,
                         int64_t* __restrict__ offs,  // [q*max_cap+j] scratch
                         int64_t* __restrict__ gbytes_out,
                         int32_t* __restrict__ overflow,
                         unsigned long long* __restrict__ bytes_out) {
  int q = blockIdx.x;
  if (q >= nq) return;
  int64_t nwin = found_out[q];
  const bool konly = qs[q].keys_only != 0;
  const uint64_t* rows = rows_out + (int64_t)q * max_cap;
  int64_t* qoffs = offs + (int64_t)q * max_cap;
  __shared__ int64_t lds[256];
  __shared__ int64_t base_s;
  if (threadIdx.x == 0) base_s = 0;
  __syncthreads();
  // phase A: exclusive offsets by chunked block scan
  for (int64_t c0 = 0; c0 < nwin; c0 += blockDim.x) {
    int64_t j = c0 + threadIdx.x;
    int64_t sz = 0;
    if (j < nwin) {
      uint64_t rt = rows[j];
      uint64_t m = (rt & ROW_TAG_DELTA ? d.meta : b.meta)[rt & ROW_MASK];
      sz = rec_bytes(meta_klen(m), konly ? 0 : meta_vlen(m));
    }
    lds[threadIdx.x] = sz;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      int64_t add = threadIdx.x >= (unsigned)off ? lds[threadIdx.x - off] : 0;
      __syncthreads();
      lds[threadIdx.x] += add;
      __syncthreads();
    }
    if (j < nwin) qoffs[j] = base_s + lds[threadIdx.x] - sz;
    __syncthreads();
    if (threadIdx.x == 0) base_s += lds[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    gbytes_out[q] = base_s;
    overflow[q] = base_s > qcap ? 1 : 0;
    atomicAdd(bytes_out, (unsigned long long)(base_s <= qcap ? base_s : 0));
  }
  // record copies happen in k_gather_copy2; this kernel only computes
  // offsets/overflow (KB_GATHER_MODE=2; mode 1 is k_gather_fused)
}

// ---- fused gather (KB_GATHER_MODE=1): offsets + copy in one kernel ---------
// One block per query. Winners are taken in chunks of GATHER_CH:
//   resolve: one thread per winner reads rows[j], then meta/rev/vo[row] — the
//     whole chunk's chains run side by side, two round trips — and a shuffle
//     scan of the record sizes leaves {row, rev, vo, klen|vlen, arena offset}
//     per winner in LDS;
//   copy: lane groups of 2^gwl lanes move records with every address taken
//     from LDS, one global round trip per record (columns/heap -> arena),
//     two records in flight per group (both records' loads before either's
//     stores).
// The overflow decision needs the query's total: a query of <= GATHER_CH
// winners (every capped bench query) is resolved once and the total falls out
// of its scan; a longer one is sized in a pass of its own first and then
// resolved chunk by chunk. Writes exactly the bytes k_gather + k_gather_copy
// wrote; the per-winner offsets live in LDS only.
constexpr int GATHER_CH = 512;  // 5 x 8 B x 512 = 20 KB of LDS
constexpr int GATHER_KR = 2;    // key u64 rounds per lane held in registers
constexpr int GATHER_VR = 4;    // value uint4 rounds per lane held in registers

// 16 B in one register quad (a native vector: stays out of scratch)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct GatherLds {
  uint64_t row[GATHER_CH];  // tagged winner row
  uint64_t rev[GATHER_CH];
  uint64_t vo[GATHER_CH];   // heap offset of the value
  uint64_t kv[GATHER_CH];   // klen | vlen << 32 (vlen 0 when keys-only)
  int64_t dst[GATHER_CH];   // record offset inside the query's arena share
  int64_t ws[16];           // block_excl_scan's per-wave sums
};

// winners [c0, c0+cn) of the query -> LDS; returns base + their bytes
__device__ __forceinline__ int64_t gather_resolve(
    const Run& rb, const Run& rd, const uint64_t* __restrict__ rows,
    int64_t c0, int cn, bool konly, int64_t base, GatherLds& L) {
  for (int s0 = 0; s0 < cn; s0 += blockDim.x) {  // block-uniform trip count
    const int s = s0 + threadIdx.x;
    uint64_t rt = 0, rv = 0, vo = 0, kv = 0;
    int64_t sz = 0;
    if (s < cn) {
      rt = rows[c0 + s];
      const Run& r = (rt & ROW_TAG_DELTA) ? rd : rb;
      const int64_t row = (int64_t)(rt & ROW_MASK);
      const uint64_t m = r.meta[row];
      rv = r.rev[row];
      vo = r.vo[row];
      const uint32_t klen = meta_klen(m), vlen = konly ? 0 : meta_vlen(m);
      kv = (uint64_t)klen | ((uint64_t)vlen << 32);
      sz = rec_bytes(klen, vlen);
    }
    int64_t tot;
    const int64_t ex = block_excl_scan<int64_t>(sz, L.ws, &tot);
    if (s < cn) {
      L.row[s] = rt;
      L.rev[s] = rv;
      L.vo[s] = vo;
      L.kv[s] = kv;
      L.dst[s] = base + ex;
    }
    base += tot;
  }
  return base;
}

// the LDS chunk's cn records -> arena
__device__ __forceinline__ void gather_copy_chunk(
    const Run& rb, const Run& rd, const uint8_t* __restrict__ spill,
    const uint8_t* __restrict__ heap, uint8_t* __restrict__ qb, int cn,
    int gwl, const GatherLds& L) {
  const int gw = 1 << gwl, gpw = 64 >> gwl;  // lanes per group, groups per wave
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int grp = lane >> gwl, gl = lane & (gw - 1);
  const int stride = (blockDim.x >> 6) * gpw;
  for (int s = w * gpw + grp; s < cn; s += 2 * stride) {
    bool ok[2];
    const uint8_t *ks[2], *vs[2];
    uint8_t* dst[2];
    uint32_t klen[2], vlen[2], kw[2], w16[2];
    uint64_t kreg[2][GATHER_KR];
    u32x4 vreg[2][GATHER_VR];
    // loads of both records first ...
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int su = s + u * stride;
      ok[u] = su < cn;
      if (!ok[u]) continue;
      const uint64_t rt = L.row[su], kv = L.kv[su];
      const Run& r = (rt & ROW_TAG_DELTA) ? rd : rb;
      ks[u] = r.keys + (int64_t)(rt & ROW_MASK) * KEYW;
      vs[u] = heap + L.vo[su];
      dst[u] = qb + L.dst[su];
      klen[u] = (uint32_t)kv;
      vlen[u] = (uint32_t)(kv >> 32);
      const uint32_t kin = klen[u] > (uint32_t)KEYW ? (uint32_t)KEYW : klen[u];
      // column rows are 96B-strided => 8-aligned; whole u64s (may round up
      // to 7B into the record's 16B key padding — always in-bounds)
      kw[u] = (kin + 7) / 8;
      w16[u] = vlen[u] >> 4;
#pragma unroll
      for (int t = 0; t < GATHER_KR; ++t) {
        const uint32_t b = gl + t * gw;
        if (b < kw[u]) kreg[u][t] = ((const uint64_t*)ks[u])[b];
      }
#pragma unroll
      for (int t = 0; t < GATHER_VR; ++t) {
        const uint32_t b = gl + t * gw;
        if (b < w16[u]) vreg[u][t] = ((const u32x4*)vs[u])[b];
      }
    }
    // ... then the stores, and whatever the register rounds did not cover
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (!ok[u]) continue;
      const int su = s + u * stride;
      if (gl == 0) {
        ((uint64_t*)dst[u])[0] = L.rev[su];
        ((uint64_t*)dst[u])[1] = (uint64_t)klen[u] | ((uint64_t)vlen[u] << 32);
      }
      uint8_t* kd = dst[u] + 16;  // records are 16B-aligned
      uint8_t* vd = kd + ((klen[u] + 15) & ~15u);
#pragma unroll
      for (int t = 0; t < GATHER_KR; ++t) {
        const uint32_t b = gl + t * gw;
        if (b < kw[u]) ((uint64_t*)kd)[b] = kreg[u][t];
      }
#pragma unroll
      for (int t = 0; t < GATHER_VR; ++t) {
        const uint32_t b = gl + t * gw;
        if (b < w16[u]) ((u32x4*)vd)[b] = vreg[u][t];
      }
      for (uint32_t b = gl + GATHER_KR * gw; b < kw[u]; b += gw)
        ((uint64_t*)kd)[b] = ((const uint64_t*)ks[u])[b];
      for (uint32_t b = gl + GATHER_VR * gw; b < w16[u]; b += gw)
        ((u32x4*)vd)[b] = ((const u32x4*)vs[u])[b];
      if (klen[u] > (uint32_t)KEYW) {  // spill tail (keys > 96B)
        const uint64_t rt = L.row[su];
        const Run& r = (rt & ROW_TAG_DELTA) ? rd : rb;
        const uint8_t* ts = spill + r.ko[rt & ROW_MASK];
        for (uint32_t t = gl; t < klen[u] - (uint32_t)KEYW; t += gw)
          kd[KEYW + t] = ts[t];
      }
      if (gl == 0)
        for (uint32_t b = w16[u] * 16; b < vlen[u]; ++b) vd[b] = vs[u][b];
    }
  }
}

__global__ __launch_bounds__(1024) void k_gather_fused(
    Run rb, Run rd, const uint8_t* __restrict__ spill,
    const uint8_t* __restrict__ heap, const uint64_t* __restrict__ rows_out,
    int64_t max_cap, const int64_t* __restrict__ found_out,
    const DevRangeQ* __restrict__ qs, int nq, uint8_t* __restrict__ gbuf,
    int64_t qcap, int64_t* __restrict__ gbytes_out,
    int32_t* __restrict__ overflow, unsigned long long* __restrict__ bytes_out,
    int gwl) {
  __shared__ GatherLds L;
  const int q = blockIdx.x;
  if (q >= nq) return;
  const int64_t nwin = found_out[q];
  const bool konly = qs[q].keys_only != 0;
  const uint64_t* rows = rows_out + (int64_t)q * max_cap;
  const bool single = nwin <= GATHER_CH;
  int64_t total = 0;
  if (single) {
    total = gather_resolve(rb, rd, rows, 0, (int)nwin, konly, 0, L);
  } else {  // size every winner first: the total decides overflow
    int64_t loc = 0;
    for (int64_t j = threadIdx.x; j < nwin; j += blockDim.x) {
      const uint64_t rt = rows[j];
      const uint64_t m =
          ((rt & ROW_TAG_DELTA) ? rd.meta : rb.meta)[rt & ROW_MASK];
      loc += rec_bytes(meta_klen(m), konly ? 0 : meta_vlen(m));
    }
    (void)block_excl_scan<int64_t>(loc, L.ws, &total);
  }
  const bool ovf = total > qcap;  // block-uniform
  if (threadIdx.x == 0) {
    gbytes_out[q] = total;
    overflow[q] = ovf ? 1 : 0;
    atomicAdd(bytes_out, (unsigned long long)(ovf ? 0 : total));
  }
  if (ovf) return;  // an overflowing query writes no record bytes
  uint8_t* qb = gbuf + (int64_t)q * qcap;
  if (single) {
    __syncthreads();
    gather_copy_chunk(rb, rd, spill, heap, qb, (int)nwin, gwl, L);
    return;
  }
  int64_t base = 0;
  for (int64_t c0 = 0; c0 < nwin; c0 += GATHER_CH) {
    const int cn = (int)(nwin - c0 < GATHER_CH ? nwin - c0 : GATHER_CH);
    base = gather_resolve(rb, rd, rows, c0, cn, konly, base, L);
    __syncthreads();
    gather_copy_chunk(rb, rd, spill, heap, qb, cn, gwl, L);
    __syncthreads();  // the next resolve overwrites the chunk
  }
}

// wave-per-record gather (KB_GATHER_MODE=2): grid (nq, cap/4), 4 records per
// 256-thread block, one 64-lane wave each — a 512B value is ONE uint4 round
// over 32 lanes and the 96B key one u64 round, with no serial record chain
// inside a lane group. Idle blocks (j >= found) retire immediately.
__global__ void k_gather_copy2(Run rb, Run rd,
                               const uint8_t* __restrict__ spill,
                               const uint8_t* __restrict__ heap,
                               const uint64_t* __restrict__ rows_out,
                               int64_t max_cap,
                               const int64_t* __restrict__ found_out,
                               const DevRangeQ* __restrict__ qs, int nq,
                               uint8_t* __restrict__ gbuf, int64_t qcap,
                               const int64_t* __restrict__ offs,
                               const int32_t* __restrict__ overflow) {
  int q = blockIdx.x;
  if (q >= nq || overflow[q]) return;
  int64_t j = (int64_t)blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (j >= found_out[q]) return;
  const bool konly = qs[q].keys_only != 0;
  const int lane = threadIdx.x & 63;
  uint64_t rt = rows_out[(int64_t)q * max_cap + j];
  bool isd = (rt & ROW_TAG_DELTA) != 0;
  int64_t row = (int64_t)(rt & ROW_MASK);
  const Run& r = isd ? rd : rb;
  uint64_t m = r.meta[row];
  uint32_t klen = meta_klen(m), vlen = konly ? 0 : meta_vlen(m);
  uint8_t* dst = gbuf + (int64_t)q * qcap + offs[(int64_t)q * max_cap + j];
  if (lane == 0) {
    *(uint64_t*)dst = r.rev[row];
    ((uint32_t*)dst)[2] = klen;
    ((uint32_t*)dst)[3] = vlen;
  }
  const uint8_t* ks = r.keys + row * KEYW;
  uint8_t* kd = dst + 16;  // records are 16B-aligned
  uint32_t kin = klen > (uint32_t)KEYW ? (uint32_t)KEYW : klen;
  for (uint32_t b = lane; b < (kin + 7) / 8; b += 64)
    ((uint64_t*)kd)[b] = ((const uint64_t*)ks)[b];
  if (klen > (uint32_t)KEYW) {  // spill tail (keys > 96B)
    const uint8_t* ts = spill + r.ko[row];
    for (uint32_t t = lane; t < klen - (uint32_t)KEYW; t += 64)
      kd[KEYW + t] = ts[t];
  }
  if (konly) return;
  const uint8_t* vs = heap + r.vo[row];
  uint8_t* vd = dst + 16 + ((klen + 15) & ~15u);
  uint32_t w16 = vlen >> 4;
  for (uint32_t b = lane; b < w16; b += 64)
    ((uint4*)vd)[b] = ((const uint4*)vs)[b];
  if (lane == 0)
    for (uint32_t b = w16 * 16; b < vlen; ++b) vd[b] = vs[b];
}

// pack used per-query regions contiguously for one D2H
__global__ void k_pack(const uint8_t* __restrict__ gbuf, int64_t qcap,
                       const int64_t* __restrict__ gbytes,
                       const int64_t* __restrict__ goffs,
                       const int32_t* __restrict__ overflow,
                       uint8_t* __restrict__ out, int nq) {
  int q = blockIdx.x;
  if (q >= nq) return;
  if (overflow[q]) return;  // nothing was gathered for this query
  int64_t bytes = gbytes[q];
  const uint4* src = (const uint4*)(gbuf + (int64_t)q * qcap);
  uint4* dst = (uint4*)(out + goffs[q]);
  int64_t words = bytes / 16;  // records are 16B-aligned (goffs too)
  for (int64_t w = threadIdx.x; w < words; w += blockDim.x) dst[w] = src[w];
}

// ---- generic exclusive scan (u64), 256-wide blocks ----------------------
__global__ void k_block_scan(const uint64_t* __restrict__ in,
                             uint64_t* __restrict__ out,
                             uint64_t* __restrict__ sums, int64_t n) {
  __shared__ uint64_t lds[256];
  int64_t base = (int64_t)blockIdx.x * 256;
  int t = threadIdx.x;
  uint64_t v = base + t < n ? in[base + t] : 0;
  lds[t] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    uint64_t add = t >= off ? lds[t - off] : 0;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  if (base + t < n) out[base + t] = lds[t] - v;
  if (t == 255) sums[blockIdx.x] = lds[255];
}

__global__ void k_add_offsets(uint64_t* __restrict__ out,
                              const uint64_t* __restrict__ block_offs, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] += block_offs[blockIdx.x];
}

// ---- compaction (compact.go + scanner.go:444-491, 566-591) --------------
__global__ void k_merge_newn(const uint64_t* __restrict__ dropx, int64_t n,
                             int64_t m, int64_t* __restrict__ out_n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *out_n = n - (int64_t)dropx[n] + m;
}

__global__ void k_fill_u64(uint64_t* a, uint64_t v, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = v;
}

__global__ void k_find_bounds(Run a, int64_t n, const uint8_t* spill,
                              const uint8_t* bkeys, const uint64_t* brevs, int nb,
                              int64_t* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  // borders are <= KEYW (validated host-side); len=KEYW orders a border
  // before any longer key sharing its full 96B prefix, which is exactly
  // lower-bound semantics
  if (i < nb)
    out[i] = d_lb_range(a, spill, 0, n,
                        QKey{bkeys + (int64_t)i * KEYW, (uint32_t)KEYW, 0, nullptr},
                        brevs[i]);
}

__global__ void k_compact_mark(const uint64_t* __restrict__ meta,
                               const uint64_t* __restrict__ rev,
                               const uint64_t* __restrict__ vo, int64_t lo,
                               int64_t hi, uint64_t compact_rev,
                               uint64_t timeout_rev, uint64_t* __restrict__ keep) {
  int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= hi) return;
  uint64_t r = rev[i], m = meta[i];
  // TTL expiry of "/events/" keys, checked BEFORE the rev skip (scanner.go:444-447)
  if (timeout_rev != 0 && (m & M_EVENTS)) {
    if (r == 0) {
      if (vo[i] <= timeout_rev) { keep[i] = 0; return; }  // scanner.go:577-581
    } else if (r <= timeout_rev) { keep[i] = 0; return; } // scanner.go:583-586
  }
  if (r > compact_rev) return;  // skipped rows survive (scanner.go:451-453)
  if (r == 0) {
    // 9B-flagged revision rows die unless objRev > compactRev (scanner.go:477-491)
    if ((m & M_FLAG9) && vo[i] <= compact_rev) keep[i] = 0;
    return;
  }
  if (m & M_TOMB) { keep[i] = 0; return; }  // scanner.go:471-475
  // superseded version: a newer same-key row with rev<=compactRev (scanner.go:464-469)
  if ((m & M_SAME_NEXT) && rev[i + 1] <= compact_rev) keep[i] = 0;
}

__global__ void k_heap_sizes(const uint64_t* __restrict__ keep,
                             const uint64_t* __restrict__ rev,
                             const uint64_t* __restrict__ meta,
                             uint64_t* __restrict__ sz, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  sz[i] = (keep[i] && rev[i] > 0) ? ((meta_vlen(meta[i]) + 15) & ~15ull) : 0;
}

__global__ void k_compact_scatter(const uint8_t* __restrict__ keysA,
                                  const uint64_t* __restrict__ metaA,
                                  const uint64_t* __restrict__ revA,
                                  const uint64_t* __restrict__ voA,
                                  const uint64_t* __restrict__ koA,
                                  const uint64_t* __restrict__ keep,
                                  const uint64_t* __restrict__ nidx,
                                  const uint64_t* __restrict__ heap_off,
                                  const uint64_t* __restrict__ spill_off,
                                  uint8_t* __restrict__ keysB,
                                  uint64_t* __restrict__ metaB,
                                  uint64_t* __restrict__ revB,
                                  uint64_t* __restrict__ voB,
                                  uint64_t* __restrict__ koB, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !keep[i]) return;
  int64_t j = (int64_t)nidx[i];
  revB[j] = revA[i];
  metaB[j] = metaA[i];
  voB[j] = revA[i] == 0 ? voA[i] : heap_off[i];
  koB[j] = meta_klen(metaA[i]) > (uint32_t)KEYW ? spill_off[i] : 0;
  const uint64_t* ks = (const uint64_t*)(keysA + i * KEYW);
  uint64_t* kd = (uint64_t*)(keysB + j * KEYW);
#pragma unroll
  for (int k = 0; k < KEYW / 8; ++k) kd[k] = ks[k];
}

// key-spill compaction (keys > KEYW): surviving tails are packed into the
// fresh spill heap, mirroring the value-heap sweep
__global__ void k_spill_sizes(const uint64_t* __restrict__ keep,
                              const uint64_t* __restrict__ meta,
                              uint64_t* __restrict__ sz, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t kl = meta_klen(meta[i]);
  sz[i] = (keep[i] && kl > (uint32_t)KEYW) ? (((uint64_t)kl - KEYW + 15) & ~15ull) : 0;
}

__global__ void k_spill_scatter(const uint64_t* __restrict__ keep,
                                const uint64_t* __restrict__ meta,
                                const uint64_t* __restrict__ koA,
                                const uint64_t* __restrict__ spill_off,
                                const uint8_t* __restrict__ spillA,
                                uint8_t* __restrict__ spillB, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (i >= n || !keep[i]) return;
  uint32_t kl = meta_klen(meta[i]);
  if (kl <= (uint32_t)KEYW) return;
  uint32_t t = kl - (uint32_t)KEYW;
  const uint8_t* src = spillA + koA[i];
  uint8_t* dst = spillB + spill_off[i];
  for (uint32_t x = lane; x < t; x += 64) dst[x] = src[x];
}

__global__ void k_heap_scatter(const uint64_t* __restrict__ keep,
                               const uint64_t* __restrict__ rev,
                               const uint64_t* __restrict__ meta,
                               const uint64_t* __restrict__ voA,
                               const uint64_t* __restrict__ heap_off,
                               const uint8_t* __restrict__ heapA,
                               uint8_t* __restrict__ heapB, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (i >= n || !keep[i] || rev[i] == 0) return;
  uint64_t bytes = (meta_vlen(meta[i]) + 15) & ~15ull;
  const uint4* src = (const uint4*)(heapA + voA[i]);
  uint4* dst = (uint4*)(heapB + heap_off[i]);
  for (uint64_t w = lane; w < bytes / 16; w += 64) dst[w] = src[w];
}

// ---- merge (memtable flush): delta ranks + scatter ----------------------
// small-insert merge (m <= 1024 new rows into an n-row run, the per-step txn
// merge), two kernels and no O(n) scratch. k_delta_rank: one wave per NEW
// row searches the run with the 64-ary wave search (m*log64(n) round trips)
// and leaves its insertion point lb[j] and whether the row there is
// (key,rev)-equal (dup[j]: a memtable revision-row replaces it).
__global__ __launch_bounds__(256) void k_delta_rank(
    Run a, int64_t n, Run dnew, int64_t m, const uint8_t* __restrict__ spill,
    int64_t* __restrict__ lbs /*[m]*/, uint32_t* __restrict__ dups /*[m]*/) {
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= m) return;  // wave-uniform
  QKey k = row_qk(dnew, spill, j);
  const uint64_t rv = dnew.rev[j];
  const int64_t lb = d_lb_wave(a, spill, n, k, rv);
  const bool dup = lb < n && a.rev[lb] == rv && rowcmp_q(a, spill, lb, k) == 0;
  if ((threadIdx.x & 63) == 0) {
    lbs[j] = lb;
    dups[j] = dup ? 1 : 0;
  }
}

__device__ __forceinline__ void copy_row(const Run& s, int64_t i,
                                         uint8_t* keysB, uint64_t* metaB,
                                         uint64_t* revB, uint64_t* voB,
                                         uint64_t* koB, int64_t out) {
  revB[out] = s.rev[i];
  metaB[out] = s.meta[i];
  voB[out] = s.vo[i];
  koB[out] = s.ko[i];
  const uint4* ks = (const uint4*)(s.keys + i * KEYW);
  uint4* kd = (uint4*)(keysB + out * KEYW);
#pragma unroll
  for (int t = 0; t < KEYW / 16; ++t) kd[t] = ks[t];
}

// k_delta_scatter: one thread per old row plus one per new row. Every block
// keeps lb[0,m) and the exclusive prefix of dup[0,m] in LDS; the m insertion
// points are monotone, so an old row finds its shift with two ~10-step
// binary searches there (dmerge.h) instead of a difference array, two
// memsets and a multi-level scan over n. New rows record their slot in
// outpos for the same_next fixup. new_n -> newn_out (s_d).
__global__ __launch_bounds__(256) void k_delta_scatter(
    Run a, int64_t n, Run dnew, int64_t m,
    const int64_t* __restrict__ lbs, const uint32_t* __restrict__ dups,
    uint64_t* __restrict__ outpos /*[m] new rows' slots*/,
    uint8_t* keysB, uint64_t* metaB, uint64_t* revB, uint64_t* voB,
    uint64_t* koB, int64_t* __restrict__ newn_out) {
  __shared__ int64_t s_lb[kbmerge::kMaxNew];
  __shared__ uint16_t s_dupx[kbmerge::kMaxNew + 4];
  __shared__ uint32_t s_ws[4];
  const int t = threadIdx.x, mi = (int)m;
  for (int x = t; x < mi; x += 256) s_lb[x] = lbs[x];
  // thread t owns dup[4t, 4t+4): 256 threads cover the 1024 possible rows
  uint32_t d[4], sum = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    d[u] = 4 * t + u < mi ? dups[4 * t + u] : 0;
    sum += d[u];
  }
  uint32_t tot;
  uint32_t run = block_excl_scan<uint32_t>(sum, s_ws, &tot);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (4 * t + u < mi) s_dupx[4 * t + u] = (uint16_t)run;
    run += d[u];
  }
  if (t == 0) s_dupx[mi] = (uint16_t)tot;  // entry m: no thread owns it at m = 1024
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * 256 + t;
  if (g < n) {
    const int64_t out = kbmerge::OldSlot(g, s_lb, s_dupx, mi);
    if (out >= 0) copy_row(a, g, keysB, metaB, revB, voB, koB, out);
  } else if (g < n + m) {
    const int j = (int)(g - n);
    const int64_t out = kbmerge::NewSlot(j, s_lb, s_dupx);
    outpos[j] = (uint64_t)out;
    copy_row(dnew, j, keysB, metaB, revB, voB, koB, out);
  }
  if (g == 0) *newn_out = kbmerge::NewCount(n, mi, s_dupx);
}

// multi-block inverted merge rank (any m into n>0 rows): each NEW row
// binary-searches the big run once — m*log2(n) probes instead of the
// forward path's n*log2(m) — and leaves a difference array v[0..n+1] whose
// prefix sum is each base row's slot shift (insertions +1 at ub_j, drops -1
// after lb_j). drop[] marks replaced base rows ((key,rev)-equal memtable
// revision-rows); dup flags go to dup[] (scanned separately to give each
// new row its drops-before count).
__global__ void k_merge_rank_inv_big(Run a, int64_t n, Run dnew, int64_t m,
                                     const uint8_t* __restrict__ spill,
                                     uint64_t* __restrict__ v /*[n+2] zeroed*/,
                                     uint64_t* __restrict__ drop /*[n] zeroed*/,
                                     uint64_t* __restrict__ dup /*[m+1] zeroed*/,
                                     uint64_t* __restrict__ lbs /*[m]*/) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  QKey k = row_qk(dnew, spill, j);
  int64_t lb = d_lb_range(a, spill, 0, n, k, dnew.rev[j]);
  bool isdup = lb < n && a.rev[lb] == dnew.rev[j] &&
               rowcmp_q(a, spill, lb, k) == 0;
  lbs[j] = (uint64_t)lb;
  if (isdup) {
    dup[j] = 1;
    drop[lb] = 1;
    atomicAdd(&v[lb + 1], (uint64_t)-1ll);
  }
  atomicAdd(&v[lb + (isdup ? 1 : 0)], 1ull);
}

// delta scatter for the big inverted path: slot = lb_j + j - dupx[j];
// rewrites lbs[j] with the final slot for the same_next fixup
__global__ void k_merge_scatter_delta2(
    Run dnew, int64_t m, const uint64_t* __restrict__ dupx /*excl scan*/,
    uint64_t* __restrict__ lbs, uint8_t* keysB, uint64_t* metaB,
    uint64_t* revB, uint64_t* voB, uint64_t* koB) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  int64_t out = (int64_t)lbs[j] + j - (int64_t)dupx[j];
  lbs[j] = (uint64_t)out;
  revB[out] = dnew.rev[j];
  metaB[out] = dnew.meta[j];
  voB[out] = dnew.vo[j];
  koB[out] = dnew.ko[j];
  const uint4* ks = (const uint4*)(dnew.keys + j * KEYW);
  uint4* kd = (uint4*)(keysB + out * KEYW);
#pragma unroll
  for (int t = 0; t < KEYW / 16; ++t) kd[t] = ks[t];
}

__global__ void k_set_newn(const uint64_t* __restrict__ dupx, int64_t n,
                           int64_t m, int64_t* __restrict__ newn_out) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    *newn_out = n + m - (int64_t)dupx[m];
}

// base-row scatter for the inverted path: slot = i + excl_scan(v)[i+1]
__global__ void k_merge_scatter_base2(
    Run a, const uint64_t* __restrict__ sv /*excl scan of v, [n+2]*/,
    const uint64_t* __restrict__ drop, uint8_t* keysB, uint64_t* metaB,
    uint64_t* revB, uint64_t* voB, uint64_t* koB, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || drop[i]) return;
  int64_t j = i + (int64_t)sv[i + 1];
  revB[j] = a.rev[i];
  metaB[j] = a.meta[i];
  voB[j] = a.vo[i];
  koB[j] = a.ko[i];
  const uint4* ks = (const uint4*)(a.keys + i * KEYW);
  uint4* kd = (uint4*)(keysB + j * KEYW);
#pragma unroll
  for (int t = 0; t < KEYW / 16; ++t) kd[t] = ks[t];
}

// same_next fixup after an inverted insert: only rows adjacent to an
// inserted slot can change (relative order of surviving base rows is
// preserved and their meta bits travel with them); recompute at out_j-1 and
// out_j for every inserted row
__global__ void k_same_next_fixup(uint8_t* __restrict__ keys,
                                  uint64_t* __restrict__ meta,
                                  const uint64_t* __restrict__ ko,
                                  const uint8_t* __restrict__ spill,
                                  int64_t new_n,
                                  const uint64_t* __restrict__ outpos,
                                  int64_t m) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * m) return;
  int64_t i = (int64_t)outpos[t >> 1] - (t & 1);
  if (i < 0 || i >= new_n) return;
  uint64_t mm = meta[i];
  bool same = i + 1 < new_n && rows_same_key(keys, meta, ko, spill, i, i + 1);
  meta[i] = same ? (mm | M_SAME_NEXT) : (mm & ~M_SAME_NEXT);
}

__global__ void k_merge_scatter_delta(
    Run a, int64_t n, Run dnew, int64_t m, const uint8_t* __restrict__ spill,
    const uint64_t* __restrict__ dropx,
    uint8_t* keysB, uint64_t* metaB, uint64_t* revB, uint64_t* voB,
    uint64_t* koB) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  QKey k = row_qk(dnew, spill, j);
  int64_t lb = d_lb_range(a, spill, 0, n, k, dnew.rev[j]);
  int64_t out = lb - (int64_t)dropx[lb] + j;
  revB[out] = dnew.rev[j];
  metaB[out] = dnew.meta[j];
  voB[out] = dnew.vo[j];
  koB[out] = dnew.ko[j];
  const uint64_t* ks = (const uint64_t*)(dnew.keys + j * KEYW);
  uint64_t* kd = (uint64_t*)(keysB + out * KEYW);
#pragma unroll
  for (int kk = 0; kk < KEYW / 8; ++kk) kd[kk] = ks[kk];
}

// single-workgroup merge for small runs (n+m <= 8192): rank, drop-scan,
// scatter and same_next in ONE launch — the multi-kernel path costs ~10
// launches plus two host syncs, which dominates small per-step delta merges.
__global__ void k_merge_small(Run src, int64_t n, Run dnew, int64_t m,
                              const uint8_t* __restrict__ spill,
                              uint8_t* __restrict__ okeys,
                              uint64_t* __restrict__ ometa,
                              uint64_t* __restrict__ orev,
                              uint64_t* __restrict__ ovo,
                              uint64_t* __restrict__ oko,
                              int64_t* __restrict__ out_n) {
  __shared__ uint16_t dropx[8193];  // exclusive drop counts (n <= 8192)
  __shared__ uint16_t partial[257];
  int t = threadIdx.x;
  const int T = blockDim.x;
  // per-thread chunk of src rows: drop flags + partial sums
  int chunk = (int)((n + T - 1) / T);
  int i0 = t * chunk;
  int i1 = min((int64_t)i0 + chunk, n);
  uint16_t cnt = 0;
  for (int i = i0; i < i1; ++i) {
    QKey k = row_qk(src, spill, i);
    int64_t lb = d_lb_range(dnew, spill, 0, m, k, src.rev[i]);
    bool drop = lb < m && dnew.rev[lb] == src.rev[i] &&
                rowcmp_q(dnew, spill, lb, k) == 0;
    dropx[i] = drop ? 1 : 0;
    cnt += drop;
  }
  partial[t] = cnt;
  __syncthreads();
  if (t == 0) {
    uint16_t acc = 0;
    for (int k = 0; k < T; ++k) { uint16_t v = partial[k]; partial[k] = acc; acc += v; }
    partial[T] = acc;
  }
  __syncthreads();
  // exclusive scan within chunk
  {
    uint16_t acc = partial[t];
    for (int i = i0; i < i1; ++i) { uint16_t v = dropx[i]; dropx[i] = acc; acc += v; }
  }
  __syncthreads();
  int64_t dropped = partial[T];
  int64_t new_n = n - dropped + m;
  if (t == 0) *out_n = new_n;
  // scatter src rows
  for (int64_t i = t; i < n; i += T) {
    QKey k = row_qk(src, spill, i);
    int64_t lb = d_lb_range(dnew, spill, 0, m, k, src.rev[i]);
    bool drop = lb < m && dnew.rev[lb] == src.rev[i] &&
                rowcmp_q(dnew, spill, lb, k) == 0;
    if (drop) continue;
    int64_t j = i - (int64_t)dropx[i] + lb;
    orev[j] = src.rev[i];
    ometa[j] = src.meta[i];
    ovo[j] = src.vo[i];
    oko[j] = src.ko[i];
    const uint64_t* ks = (const uint64_t*)(src.keys + i * KEYW);
    uint64_t* kd = (uint64_t*)(okeys + j * KEYW);
#pragma unroll
    for (int k2 = 0; k2 < KEYW / 8; ++k2) kd[k2] = ks[k2];
  }
  // scatter new rows
  for (int64_t j = t; j < m; j += T) {
    QKey k = row_qk(dnew, spill, j);
    int64_t lb = d_lb_range(src, spill, 0, n, k, dnew.rev[j]);
    int64_t dpx = lb < n ? dropx[lb] : (int64_t)dropped;
    int64_t o = lb - dpx + j;
    orev[o] = dnew.rev[j];
    ometa[o] = dnew.meta[j];
    ovo[o] = dnew.vo[j];
    oko[o] = dnew.ko[j];
    const uint64_t* ks = (const uint64_t*)(dnew.keys + j * KEYW);
    uint64_t* kd = (uint64_t*)(okeys + o * KEYW);
#pragma unroll
    for (int k2 = 0; k2 < KEYW / 8; ++k2) kd[k2] = ks[k2];
  }
  __syncthreads();
  // same_next over the merged rows (full-key equality incl. spill tails)
  for (int64_t i = t; i < new_n; i += T) {
    bool same = i + 1 < new_n &&
                rows_same_key(okeys, ometa, oko, spill, i, i + 1);
    ometa[i] = same ? (ometa[i] | M_SAME_NEXT) : (ometa[i] & ~M_SAME_NEXT);
  }
}

// ---- watch fan-out over the DEVICE-RESIDENT event log -------------------
// (watch.go:119-159 per-watcher predicate; north_star: "GPU-resident event
// log"). The log is a ring of (key96, rev) columns in HBM, pushed once per
// event batch; the fan-out filter stages each batch through LDS and tests
// all watchers against it; catch-up (Ring.FindEvents, ring.go:84-118) is a
// thread-per-event scan over the resident ring. Values/full events stay in
// the host ring for materialization at poll time — matching the reference,
// which fans out shared batch POINTERS and filters in the consumer
// (watcherhub.go:78-100, watch.go:119-159).

// one 64-thread block per (64-watcher slice x 64-event chunk): at 10k
// watchers / 512 events that is 157x8 = 1256 single-wave blocks (the old
// one-thread-per-watcher shape launched only W/256 = 40 blocks and left the
// chip idle). Each block stages its event chunk (key96+rev, 6.5 KB) in LDS;
// each thread (= one watcher) tests the 64 events and emits exactly one
// bitmap word — no atomics, no cross-wave syncs, no ballot needed.
__global__ void k_watch_filter2(const uint8_t* __restrict__ er_keys,
                                const uint64_t* __restrict__ er_rev,
                                int64_t ring_cap, int64_t base_seq,
                                int64_t count,
                                const uint8_t* __restrict__ wpfx,
                                const uint32_t* __restrict__ wplen,
                                const uint64_t* __restrict__ wfrom,
                                const uint32_t* __restrict__ wlive, int64_t W,
                                uint64_t* __restrict__ bitmap, int64_t words) {
  __shared__ uint64_t lkeys[64 * (KEYW / 8)];
  __shared__ uint64_t lrev[64];
  const int64_t w = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.y << 6;
  const int64_t cn = min((int64_t)64, count - c0);
  // stage the chunk: consecutive threads load consecutive u64s (ring slots
  // may wrap, so the slot is recomputed per element)
  for (int64_t v = threadIdx.x; v < cn * (KEYW / 8); v += 64) {
    int64_t j = v / (KEYW / 8), k = v % (KEYW / 8);
    int64_t slot = (base_seq + c0 + j) % ring_cap;
    lkeys[v] = ((const uint64_t*)(er_keys + slot * KEYW))[k];
  }
  if (threadIdx.x < cn) {
    int64_t slot = (base_seq + c0 + threadIdx.x) % ring_cap;
    lrev[threadIdx.x] = er_rev[slot];
  }
  __syncthreads();
  if (w >= W) return;
  uint64_t acc = 0;
  if (wlive[w]) {
    const uint8_t* pfx = wpfx + w * KEYW;
    const uint32_t plen = wplen[w];
    const uint64_t from = wfrom[w];
    for (int64_t j = 0; j < cn; ++j) {
      bool ok = lrev[j] >= from;  // filterByRevision (watch.go:152-158)
      if (ok) {                   // filterByPrefix (watch.go:139-149)
        const uint8_t* k = (const uint8_t*)(lkeys + j * (KEYW / 8));
        uint32_t b = 0;
        for (; b + 8 <= plen; b += 8)
          if (*(const uint64_t*)(pfx + b) != *(const uint64_t*)(k + b)) break;
        if (b + 8 <= plen) ok = false;
        else
          for (; b < plen && ok; ++b)
            if (pfx[b] != k[b]) ok = false;
      }
      if (ok) acc |= 1ull << j;
    }
  }
  bitmap[w * words + blockIdx.y] = acc;
}

// catch-up: ONE watcher's prefix over a resident ring span, thread-per-event
__global__ void k_watch_catchup(const uint8_t* __restrict__ er_keys,
                                const uint64_t* __restrict__ er_rev,
                                int64_t ring_cap, int64_t base_seq,
                                int64_t count, const uint8_t* __restrict__ pfx,
                                uint32_t plen, uint64_t from_rev,
                                uint64_t* __restrict__ words) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int lane = threadIdx.x & 63;
  bool ok = false;
  if (e < count) {
    int64_t slot = (base_seq + e) % ring_cap;
    ok = er_rev[slot] >= from_rev;
    if (ok) {
      const uint8_t* k = er_keys + slot * KEYW;
      uint32_t b = 0;
      for (; b + 8 <= plen; b += 8)
        if (*(const uint64_t*)(pfx + b) != *(const uint64_t*)(k + b)) break;
      if (b + 8 <= plen) ok = false;
      else
        for (; b < plen && ok; ++b)
          if (pfx[b] != k[b]) ok = false;
    }
  }
  uint64_t b = __ballot(ok);
  if (lane == 0 && e < count) words[e >> 6] = b;
}

// ---- batched watch poll: serialize deliveries on the device --------------
// (kb_watch_poll_batch). Next to (key96, rev) the event ring
// carries er_poff/er_plen: where each event's wire record (i32 type | u64
// rev | u64 kv_rev | u32 klen | key | u32 vlen | val, serialized ONCE by the
// host at pump time) sits in the payload byte ring. A delivery is then a
// byte copy: one wave per bitmap ref, 4 waves per block.

__device__ __forceinline__ uint64_t wp_shfl64(uint64_t v, int src) {
  uint32_t lo = __shfl((uint32_t)v, src, 64);
  uint32_t hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}

// inclusive wave prefix sum (64 lanes)
__device__ __forceinline__ uint64_t wp_scan64(uint64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t lo = __shfl_up((uint32_t)v, d, 64);
    uint32_t hi = __shfl_up((uint32_t)(v >> 32), d, 64);
    if (lane >= d) v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// lane l takes bit l of each word; a wave reduction yields {bytes, count}
__global__ __launch_bounds__(256) void k_wpoll_size(
    const WpollRef* __restrict__ refs, int64_t nrefs,
    const uint32_t* __restrict__ er_plen, int64_t ring_cap,
    WpollSize* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nrefs) return;  // wave-uniform
  const WpollRef* ref = refs + r;
  const int64_t base = ref->base;
  const int32_t count = ref->count;
  uint64_t bytes = 0;
  uint32_t cnt = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (c * 64 + lane < count && ((ref->words[c] >> lane) & 1)) {
      bytes += er_plen[(base + c * 64 + lane) % ring_cap];
      ++cnt;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    uint32_t lo = __shfl_xor((uint32_t)bytes, d, 64);
    uint32_t hi = __shfl_xor((uint32_t)(bytes >> 32), d, 64);
    bytes += ((uint64_t)hi << 32) | lo;
    cnt += __shfl_xor(cnt, d, 64);
  }
  if (lane == 0) {
    WpollSize s;
    s.bytes = bytes;
    s.count = cnt;
    s._pad = 0;
    out[r] = s;
  }
}

// wave-cooperative copy of one record: src is 16-byte aligned (payload ring
// placement), dst is arbitrarily aligned (the wire format is packed). The
// body goes out as ALIGNED 16-byte destination stores, each built from two
// aligned 16-byte source loads by a funnel shift; the up-to-15 head bytes
// before the first aligned destination address and the up-to-15 tail bytes
// go out as single byte stores. Neighbouring records are written by other
// waves and may share a destination dword/qword with this one, so no wide
// store ever reaches outside [dst, dst+len).
__device__ __forceinline__ void wp_copy_record(const uint8_t* __restrict__ src,
                                               uint8_t* __restrict__ dst,
                                               uint32_t len, int lane) {
  uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
  if (head > len) head = len;
  if ((uint32_t)lane < head) dst[lane] = src[lane];
  const uint32_t nq = (len - head) >> 4;      // full aligned 16 B stores
  const uint32_t shb = head & 15;             // src misalignment of the body
  const uint32_t wsh = shb >> 2, bsh = (shb & 3) * 8;
  const uint4* s4 = (const uint4*)(src + (head & ~15u));  // == src
  uint4* d4 = (uint4*)(dst + head);
  for (uint32_t i = lane; i < nq; i += 64) {
    uint4 a = s4[i];
    // the second source quad is needed (and guaranteed inside the record's
    // 16 B-aligned extent) only when the body is misaligned
    uint4 b = shb ? s4[i + 1] : make_uint4(0, 0, 0, 0);
    uint32_t t0, t1, t2, t3, t4;
    switch (wsh) {  // wave-uniform: no indexed register array, no scratch
      case 0: t0 = a.x; t1 = a.y; t2 = a.z; t3 = a.w; t4 = b.x; break;
      case 1: t0 = a.y; t1 = a.z; t2 = a.w; t3 = b.x; t4 = b.y; break;
      case 2: t0 = a.z; t1 = a.w; t2 = b.x; t3 = b.y; t4 = b.z; break;
      default: t0 = a.w; t1 = b.x; t2 = b.y; t3 = b.z; t4 = b.w; break;
    }
    uint4 o;
    o.x = (uint32_t)((((uint64_t)t1 << 32) | t0) >> bsh);
    o.y = (uint32_t)((((uint64_t)t2 << 32) | t1) >> bsh);
    o.z = (uint32_t)((((uint64_t)t3 << 32) | t2) >> bsh);
    o.w = (uint32_t)((((uint64_t)t4 << 32) | t3) >> bsh);
    d4[i] = o;
  }
  const uint32_t done = head + (nq << 4);
  if ((uint32_t)lane < len - done) dst[done + lane] = src[done + lane];
}

// one wave per ref: recompute per-event offsets with a wave prefix sum in
// (word, lane) order == ascending revision == WatchPollWire's order, then
// copy each record, the whole wave cooperating on one record at a time
__global__ __launch_bounds__(256) void k_wpoll_emit(
    const WpollRef* __restrict__ refs, const uint64_t* __restrict__ ref_off,
    int64_t nrefs, const uint64_t* __restrict__ er_poff,
    const uint32_t* __restrict__ er_plen, int64_t ring_cap,
    const uint8_t* __restrict__ pay, int64_t pay_cap,
    uint8_t* __restrict__ arena, int64_t arena_cap) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nrefs) return;  // wave-uniform
  const WpollRef* ref = refs + r;
  const int64_t base = ref->base;
  const int32_t count = ref->count;
  uint64_t run = ref_off[r];  // destination of the next word's first record
  for (int c = 0; c < 8 && c * 64 < count; ++c) {
    const bool bit = c * 64 + lane < count && ((ref->words[c] >> lane) & 1);
    uint64_t poff = 0;
    uint32_t plen = 0;
    if (bit) {
      int64_t slot = (base + c * 64 + lane) % ring_cap;
      poff = er_poff[slot];
      plen = er_plen[slot];
    }
    const uint64_t incl = wp_scan64(plen, lane);
    const uint64_t doff = run + incl - plen;
    uint64_t mask = __ballot(bit);
    while (mask) {  // wave-uniform
      const int j = __builtin_ctzll(mask);
      mask &= mask - 1;
      const uint64_t so = wp_shfl64(poff, j);
      const uint64_t dd = wp_shfl64(doff, j);
      const uint32_t ln = __shfl(plen, j, 64);
      // defensive bounds: a record the host did not place inside the ring
      // or the arena is skipped, never copied out of bounds
      if (so + (((uint64_t)ln + 15) & ~15ull) > (uint64_t)pay_cap ||
          dd + ln > (uint64_t)arena_cap)
        continue;
      wp_copy_record(pay + so, arena + dd, ln, lane);
    }
    run += wp_shfl64(incl, 63);
  }
}

// ---- batched List (kb_list_batch) -------------------------
// The scan is k_range_bounds + k_range_scan2 unchanged (cap = limit+1): the
// tagged winner rows of query q sit in rows_m[q*max_cap ..], found_out[q] of
// them. k_list_size turns them into wire sizes, k_list_emit into wire bytes
// {u64 rev; u32 klen; key; u32 vlen; val} packed back to back.

// one 256-thread block per query: the first min(found, limit) winners, one
// meta word each (8 B per winner, no key or value column), exclusive wire
// offsets by wave scans chained through LDS
__global__ __launch_bounds__(256) void k_list_size(
    Run b, Run d, int64_t n, int64_t dn,
    const uint64_t* __restrict__ rows_m, int64_t max_cap,
    const int64_t* __restrict__ found_out,
    const int64_t* __restrict__ total_out,
    const DevRangeQ* __restrict__ qs, int nq,
    uint64_t* __restrict__ offs, ListSize* __restrict__ out) {
  const int q = blockIdx.x;
  if (q >= nq) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __shared__ uint64_t wsum[4];
  int64_t found = found_out[q];
  if (found < 0) found = 0;
  if (found > max_cap) found = max_cap;
  const int64_t cap = qs[q].cap;  // limit+1; <= 0 unbounded
  const bool more = cap > 0 && found >= cap;      // range.go:168-171
  const int64_t take = more ? cap - 1 : found;    // the cut to `limit`
  // the table held the whole answer unless List's own continuation test
  // (written >= cap || total > written) fires for an unbounded query, or
  // the cap never fitted the table
  const bool partial = cap > 0 ? cap > max_cap
                               : (found >= max_cap || total_out[q] > found);
  const bool konly = qs[q].keys_only != 0;
  const uint64_t* rows = rows_m + (int64_t)q * max_cap;
  uint64_t* qoffs = offs + (int64_t)q * max_cap;
  uint64_t base = 0;  // block-uniform running section size
  for (int64_t c0 = 0; c0 < take; c0 += 256) {
    const int64_t j = c0 + threadIdx.x;
    uint64_t sz = 0;
    if (j < take) {
      const uint64_t rt = rows[j];
      const bool isd = (rt & ROW_TAG_DELTA) != 0;
      const int64_t row = (int64_t)(rt & ROW_MASK);
      if (row < (isd ? dn : n)) {
        const uint64_t m = (isd ? d.meta : b.meta)[row];
        sz = 16 + (uint64_t)meta_klen(m) + (konly ? 0 : meta_vlen(m));
      }
    }
    const uint64_t incl = wp_scan64(sz, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint64_t woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < w) woff += wsum[k];
      tot += wsum[k];
    }
    if (j < take) qoffs[j] = base + woff + incl - sz;
    base += tot;
    __syncthreads();  // wsum reused by the next chunk
  }
  if (threadIdx.x == 0) {
    ListSize s;
    s.bytes = base;
    s.count = (uint32_t)take;
    s.flags = (more ? LS_MORE : 0) | (partial ? LS_PARTIAL : 0);
    out[q] = s;
  }
}

// one wave per winner record, flat over the round's records: wave g finds
// its query by a binary search over cum[] (records before each query), so
// skewed batches leave no idle blocks. The destination sec_base[q] + offs is
// arbitrarily aligned (the wire is packed); the three sources (96 B key
// column row, key-spill tail, value heap) are 16 B aligned and padded to 16,
// which is what wp_copy_record needs. Store-hazard rule of §3.5: nothing
// wider than a byte leaves [dst, dst+reclen); the 12+4 header bytes go out
// as byte stores. A record that would leave the arena, or whose source lies
// outside the run / heap, is skipped, never written.
__global__ __launch_bounds__(256) void k_list_emit(
    Run rb, Run rd, int64_t n, int64_t dn,
    const uint8_t* __restrict__ spill, int64_t spill_used,
    const uint8_t* __restrict__ heap, int64_t heap_used,
    const uint64_t* __restrict__ rows_m, int64_t max_cap,
    const DevRangeQ* __restrict__ qs, int nq,
    const uint64_t* __restrict__ offs, const uint64_t* __restrict__ sec_base,
    const uint64_t* __restrict__ cum, uint8_t* __restrict__ arena,
    int64_t arena_cap) {
  const int lane = threadIdx.x & 63;
  const uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= cum[nq]) return;  // wave-uniform
  int lo = 0, hi = nq;       // cum[lo] <= g < cum[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] <= g) lo = mid; else hi = mid;
  }
  const int q = lo;
  const uint64_t j = g - cum[q];
  if (j >= (uint64_t)max_cap) return;
  const uint64_t rt = rows_m[(int64_t)q * max_cap + (int64_t)j];
  const bool isd = (rt & ROW_TAG_DELTA) != 0;
  const int64_t row = (int64_t)(rt & ROW_MASK);
  if (row >= (isd ? dn : n)) return;
  const Run& r = isd ? rd : rb;
  const uint64_t m = r.meta[row];
  const uint32_t klen = meta_klen(m);
  const uint32_t vlen = qs[q].keys_only ? 0 : meta_vlen(m);
  const uint64_t dd = sec_base[q] + offs[(int64_t)q * max_cap + (int64_t)j];
  const uint64_t reclen = 16 + (uint64_t)klen + vlen;
  if (dd > (uint64_t)arena_cap || reclen > (uint64_t)arena_cap - dd) return;
  uint8_t* dst = arena + dd;
  const uint64_t rev = r.rev[row];
  if (lane < 8) dst[lane] = (uint8_t)(rev >> (8 * lane));
  else if (lane < 12) dst[lane] = (uint8_t)(klen >> (8 * (lane - 8)));
  else if (lane < 16) dst[klen + lane] = (uint8_t)(vlen >> (8 * (lane - 12)));
  const uint32_t kin = klen > (uint32_t)KEYW ? (uint32_t)KEYW : klen;
  wp_copy_record(r.keys + row * KEYW, dst + 12, kin, lane);
  if (klen > (uint32_t)KEYW) {  // spill tail (keys > 96B)
    const uint64_t ko = r.ko[row];
    const uint32_t tl = klen - (uint32_t)KEYW;
    if ((ko & 15) == 0 && ko + ((tl + 15) & ~15u) <= (uint64_t)spill_used)
      wp_copy_record(spill + ko, dst + 12 + KEYW, tl, lane);
  }
  if (vlen) {
    const uint64_t vo = r.vo[row];
    if ((vo & 15) == 0 &&
        vo + (((uint64_t)vlen + 15) & ~15ull) <= (uint64_t)heap_used)
      wp_copy_record(heap + vo, dst + 16 + klen, vlen, lane);
  }
}

// ---- batched point read (kb_get_batch) ---------------------
// k_get_find resolves each query to a tagged row, k_get_plan turns the rows
// into the reply's finished directory entries and per-query arena offsets,
// k_get_emit packs the value bytes back to back in the arena. k_get2 and its
// callers are not involved.

constexpr uint64_t GET_ROW_NONE = ~0ull;  // no row (key, rev <= R) exists

// one wave per query, four per block: the search of k_get2 (delta first,
// then base; the delta run wins when it has any row of the key <= R)
__global__ __launch_bounds__(256) void k_get_find(
    Run b, Run d, int64_t n, int64_t dn, const uint8_t* __restrict__ spill,
    const uint8_t* __restrict__ qtails, const DevGetQ* __restrict__ qs, int nq,
    uint64_t* __restrict__ otag, uint64_t* __restrict__ orev,
    uint64_t* __restrict__ ometa) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (q >= nq) return;  // wave-uniform
  const DevGetQ& Q = qs[q];
  const QKey qk{Q.key, Q.klen, Q.ko, qtails};
  // upper_bound(key, R) == lower_bound(key, R + 1), saturating
  const uint64_t nr = Q.read_rev == UINT64_MAX ? UINT64_MAX : Q.read_rev + 1;
  uint64_t tag = GET_ROW_NONE;
  if (dn > 0) {
    const int64_t ub = d_lb_wave(d, spill, dn, qk, nr);
    if (ub > 0 && d.rev[ub - 1] >= 1 && rowcmp_q(d, spill, ub - 1, qk) == 0)
      tag = ROW_TAG_DELTA | (uint64_t)(ub - 1);
  }
  if (tag == GET_ROW_NONE) {
    const int64_t ub = d_lb_wave(b, spill, n, qk, nr);
    if (ub > 0 && b.rev[ub - 1] >= 1 && rowcmp_q(b, spill, ub - 1, qk) == 0)
      tag = (uint64_t)(ub - 1);
  }
  if (lane != 0) return;
  otag[q] = tag;
  if (tag == GET_ROW_NONE) {
    orev[q] = 0;
    ometa[q] = 0;
  } else {
    const Run& r = (tag & ROW_TAG_DELTA) ? d : b;
    const int64_t row = (int64_t)(tag & ROW_MASK);
    orev[q] = r.rev[row];
    ometa[q] = r.meta[row];
  }
}

// one 256-thread block per sub-batch, 256 queries per pass: has_kv and vlen
// per query, the exclusive scan of vlen (wave scans chained through LDS) as
// arena offsets, and the reply's 32-byte directory entries in final form.
// hdr = {u64 total; u64 skipped; nq x {i32 status; i32 has_kv; u64
// header_rev; u64 mod_rev; u64 vlen}}; the skipped counter of k_get_emit is
// zeroed here, one launch ahead of its first increment.
__global__ __launch_bounds__(256) void k_get_plan(
    const uint64_t* __restrict__ tag, const uint64_t* __restrict__ rev,
    const uint64_t* __restrict__ meta, int nq, int no_values,
    uint64_t committed, uint64_t* __restrict__ aoff,
    uint64_t* __restrict__ hdr) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __shared__ uint64_t wsum[4];
  uint64_t base = 0;  // block-uniform running total
  for (int c0 = 0; c0 < nq; c0 += 256) {
    const int q = c0 + threadIdx.x;
    uint64_t vlen = 0, mod = 0;
    bool has = false;
    if (q < nq) {
      const uint64_t m = meta[q];
      has = tag[q] != GET_ROW_NONE && !(m & M_TOMB);
      if (has) {
        mod = rev[q];
        vlen = no_values ? 0 : meta_vlen(m);
      }
    }
    const uint64_t incl = wp_scan64(vlen, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint64_t woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < w) woff += wsum[k];
      tot += wsum[k];
    }
    if (q < nq) {
      aoff[q] = base + woff + incl - vlen;
      uint64_t* e = hdr + 2 + 4 * (int64_t)q;
      e[0] = (uint64_t)(has ? 1 : 0) << 32;  // status KB_OK | has_kv
      e[1] = mod > committed ? mod : committed;
      e[2] = mod;
      e[3] = vlen;
    }
    base += tot;
    __syncthreads();  // wsum reused by the next pass
  }
  if (threadIdx.x == 0) {
    hdr[0] = base;
    hdr[1] = 0;
  }
}

// one 256-thread block per query: wave w copies the 4 KiB chunks w, w + 4,
// ... of the value from the heap to arena + aoff[q]. vo is 16 B aligned and
// the value padded to 16 in the heap, chunk starts are multiples of 16 from
// there, so every chunk is a legal wp_copy_record call; its 16-byte stores
// stay inside the chunk's own destination range and byte stores cover the
// edges (§3.5 store-hazard rule: neighbouring values are other blocks').
// A query with no bytes, a row or heap extent out of range, a misaligned vo
// or a destination leaving the arena is skipped whole and counted.
__global__ __launch_bounds__(256) void k_get_emit(
    Run rb, Run rd, int64_t n, int64_t dn, const uint8_t* __restrict__ heap,
    int64_t heap_used, const uint64_t* __restrict__ tag,
    const uint64_t* __restrict__ aoff, const uint64_t* __restrict__ hdr,
    int nq, uint8_t* __restrict__ arena, int64_t arena_cap,
    unsigned long long* __restrict__ skipped) {
  const int q = blockIdx.x;
  if (q >= nq) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t vlen = hdr[2 + 4 * (int64_t)q + 3];
  const uint64_t t = tag[q];
  const uint64_t dd = aoff[q];
  bool ok = vlen != 0 && t != GET_ROW_NONE;
  uint64_t vo = 0;
  if (ok) {
    const bool isd = (t & ROW_TAG_DELTA) != 0;
    const int64_t row = (int64_t)(t & ROW_MASK);
    ok = row < (isd ? dn : n);
    if (ok) vo = (isd ? rd.vo : rb.vo)[row];
  }
  ok = ok && (vo & 15) == 0 && vo <= (uint64_t)heap_used &&
       ((vlen + 15) & ~15ull) <= (uint64_t)heap_used - vo &&
       dd <= (uint64_t)arena_cap && vlen <= (uint64_t)arena_cap - dd;
  if (!ok) {  // block-uniform
    if (threadIdx.x == 0) atomicAdd(skipped, 1ull);
    return;
  }
  const uint8_t* src = heap + vo;
  uint8_t* dst = arena + dd;
  for (uint64_t c = (uint64_t)w << 12; c < vlen; c += 4ull << 12) {
    const uint64_t left = vlen - c;
    wp_copy_record(src + c, dst + c, left < 4096 ? (uint32_t)left : 4096u, lane);
  }
}

// ---- batched Count (kb_count_batch) --------------------------
// Counting needs no order: the winner predicate is a pure function of row i,
// row i + 1, the shadow column and R. k_range_bounds (unchanged) resolves the
// four run bounds per query, k_count_plan numbers the T-row tiles of the
// launch's 2 * nq segments (cplan.h), k_count_tiles spreads the tiles over the
// chip and adds each tile's winners into its query's counter. k_range_scan2
// and scan_run_winners are not involved.
//
// chdr = {u64 tiles done; u64 rows done; u64 tiles planned; u64 rows planned;
// nq x u64 count}: the block the host reads back.
constexpr int COUNT_HDR = 4;

// one 256-thread block per launch, 256 segments per pass: tiles per segment
// and their exclusive scan (wave scans chained through LDS) into pfx[2 * nq
// + 1]; the planned totals; the counters k_count_tiles adds to are zeroed
// here, one launch ahead of their first increment.
__global__ __launch_bounds__(256) void k_count_plan(
    const int64_t* __restrict__ bounds, int nq, int64_t T,
    uint64_t* __restrict__ pfx, uint64_t* __restrict__ chdr) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nseg = 2 * nq;
  __shared__ uint64_t wsum[4], wrows[4];
  uint64_t base = 0, rows_all = 0;  // block-uniform running totals
  for (int c0 = 0; c0 < nseg; c0 += 256) {
    const int s = c0 + threadIdx.x;
    uint64_t tiles = 0, rows = 0;
    if (s < nseg) {
      const int64_t lo = kbcount::SegLo(bounds, s), hi = kbcount::SegHi(bounds, s);
      tiles = kbcount::SegTiles(lo, hi, T);
      rows = (uint64_t)kbcount::SegRows(lo, hi);
    }
    const uint64_t incl = wp_scan64(tiles, lane);
    const uint64_t rincl = wp_scan64(rows, lane);
    if (lane == 63) { wsum[w] = incl; wrows[w] = rincl; }
    __syncthreads();
    uint64_t woff = 0, tot = 0, rtot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < w) woff += wsum[k];
      tot += wsum[k];
      rtot += wrows[k];
    }
    if (s < nseg) pfx[s] = base + woff + incl - tiles;
    base += tot;
    rows_all += rtot;
    __syncthreads();  // wsum / wrows reused by the next pass
  }
  for (int q = threadIdx.x; q < nq; q += 256) chdr[COUNT_HDR + q] = 0;
  if (threadIdx.x == 0) {
    pfx[nseg] = base;
    chdr[0] = 0;
    chdr[1] = 0;
    chdr[2] = base;
    chdr[3] = rows_all;
  }
}

// fixed grid (sized by the CU count: the tile total is known only on the
// device), blocks grid-stride over tile ids. A block maps its tile through
// cplan.h, its 4 waves take the 64-row slices of [r0, r1) round-robin: rev /
// meta / shadow 8-byte streams, no key bytes. The rev[i + 1] load is guarded
// by the end of the SEGMENT, not of the tile: the last row of a tile looks
// into the next tile. The shadow column applies to the base run only and
// only while the delta holds rows, as in scan_run_winners. Per tile: ballot
// + popcount per wave, a block reduction through LDS, ONE 64-bit atomicAdd
// into the query's counter (integer adds commute: exact in any order). A tile
// whose rows leave its run is skipped and not counted as done, which the
// host reports as an error.
__global__ __launch_bounds__(256) void k_count_tiles(
    Run b, int64_t n, Run d, int64_t dn, const uint64_t* __restrict__ shadow,
    const DevRangeQ* __restrict__ qs, int nq,
    const int64_t* __restrict__ bounds, const uint64_t* __restrict__ pfx,
    int64_t T, uint64_t* __restrict__ chdr) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nseg = 2 * nq;
  __shared__ uint32_t wcnt[4];
  const uint64_t total = pfx[nseg];
  uint64_t done = 0, rows_done = 0;  // thread 0's tallies of this block
  for (uint64_t t = blockIdx.x; t < total; t += gridDim.x) {
    const kbcount::Tile tl = kbcount::MapTile(bounds, pfx, nseg, t, T);
    const bool isd = tl.run != 0;
    const int64_t run_n = isd ? dn : n;
    if (tl.r0 < 0 || tl.r0 >= tl.r1 || tl.r1 > tl.hi || tl.hi > run_n)
      continue;  // block-uniform
    const uint64_t* __restrict__ rev = isd ? d.rev : b.rev;
    const uint64_t* __restrict__ meta = isd ? d.meta : b.meta;
    const uint64_t* __restrict__ sh = (!isd && dn > 0) ? shadow : nullptr;
    const uint64_t R = qs[tl.query].read_rev;
    const int64_t seg_hi = tl.hi;
    uint32_t cnt = 0;  // wave-uniform
#pragma unroll 4
    for (int64_t i0 = tl.r0 + ((int64_t)w << 6); i0 < tl.r1; i0 += 256) {
      const int64_t i = i0 + lane;
      bool win = false;
      if (i < tl.r1) {
        const uint64_t rv = rev[i], m = meta[i];
        const uint64_t rvn = (i + 1 < seg_hi) ? rev[i + 1] : 0;
        const uint64_t s = sh ? sh[i] : UINT64_MAX;
        if (rv > 0 && rv <= R && !(m & M_TOMB) && !(s != UINT64_MAX && s <= R))
          win = !(m & M_SAME_NEXT) || rvn > R;
      }
      cnt += (uint32_t)__popcll(__ballot(win));
    }
    if (lane == 0) wcnt[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint64_t c = (uint64_t)wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
      if (c)
        atomicAdd((unsigned long long*)&chdr[COUNT_HDR + tl.query],
                  (unsigned long long)c);
      done += 1;
      rows_done += (uint64_t)(tl.r1 - tl.r0);
    }
    __syncthreads();  // wcnt reused by the next tile
  }
  if (threadIdx.x == 0 && done) {
    atomicAdd((unsigned long long*)&chdr[0], (unsigned long long)done);
    atomicAdd((unsigned long long*)&chdr[1], (unsigned long long)rows_done);
  }
}

// ------------------------------------------------------------------ Impl ---

struct Slab::Impl {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t max_rows = 0, heap_cap = 0;
  int64_t n = 0, heap_used_ = 0;

  struct Col {
    uint8_t* keys = nullptr;
    uint64_t *meta = nullptr, *rev = nullptr, *vo = nullptr, *ko = nullptr;
    Run run() const { return Run{keys, meta, rev, vo, ko}; }
  };
  Col A, B;
  Col DA, DB;            // delta-run ping-pong
  int64_t dn = 0;        // delta-run rows
  int64_t delta_cap = 0; // rows per delta buffer
  uint8_t *heapA = nullptr, *heapB = nullptr;
  // key-spill heap (tails of keys > KEYW), shared by base+delta; compacted
  // with the rows in Compact
  uint8_t *spillA = nullptr, *spillB = nullptr;
  int64_t spill_cap = 0, spill_used_ = 0;
  // per-batch query-tail buffer (bounds/get keys > KEYW)
  // d_qtails/d_qs/d_gq are what the kernels of the CURRENT batch read: the
  // *_own buffers for a batch uploaded by the per-call entry points (every
  // one of them passes through ensure_qtails first), slices of the step
  // staging block for a staged bench step (StepStageCommit)
  uint8_t* d_qtails = nullptr;
  uint8_t* d_qtails_own = nullptr;
  int64_t qt_cap = 0;
  bool ensure_qtails(const std::string& qt, std::string* err) {
    if ((int64_t)qt.size() > qt_cap) {
      if (d_qtails_own) (void)hipFree(d_qtails_own);
      d_qtails_own = nullptr;
      qt_cap = 0;
      int64_t cap = (int64_t)qt.size() * 2 + 4096;
      HIP_CHECK(hipMalloc(&d_qtails_own, cap));
      qt_cap = cap;
    }
    d_qtails = d_qtails_own;
    d_qs = d_qs_own;
    d_gq = d_gq_own;
    if (!qt.empty())
      HIP_CHECK(hipMemcpyAsync(d_qtails, qt.data(), qt.size(),
                               hipMemcpyHostToDevice, stream));
    return true;
  }

  // scan scratch (u64, shared across ops)
  uint64_t* shadow = nullptr;  // [max_rows] base shadow-revision column
  uint64_t* d_outpos = nullptr;  // small insert: [1024] dest slots | lb | dup
  // big inverted merge scratch: dup flags / their scan / new-row lower
  // bounds (then final slots), all m-sized, grown on demand
  uint64_t *d_mdup = nullptr, *d_mdupx = nullptr, *d_mlbs = nullptr;
  uint8_t* h_uploads[2] = {nullptr, nullptr};  // pinned delta-upload mirrors
  hipEvent_t ev_up[2] = {nullptr, nullptr};
  int up_idx = 0;
  DevRangeQ* h_qs[2] = {nullptr, nullptr};  // pinned query-upload mirrors
  hipEvent_t ev_qs[2] = {nullptr, nullptr};
  int qs_idx = 0;
  // pinned double-buffered staging for heap/spill appends: the old pageable
  // copies needed a FULL stream sync per call (in the pipelined bench that
  // waited out the previous step's scan+gather kernels)
  uint8_t* h_blob[2] = {nullptr, nullptr};
  int64_t h_blob_cap[2] = {0, 0};
  hipEvent_t ev_blob[2] = {nullptr, nullptr};
  int blob_idx = 0;
  uint8_t* stage_blob(const void* src, int64_t len, std::string* err) {
    int slot = blob_idx ^= 1;
    if (!ev_blob[slot]) {
      hipError_t _e = hipEventCreate(&ev_blob[slot]);
      if (_e != hipSuccess) { if (err) *err = hipGetErrorString(_e); return nullptr; }
    }
    (void)hipEventSynchronize(ev_blob[slot]);
    if (len > h_blob_cap[slot]) {
      if (h_blob[slot]) (void)hipHostFree(h_blob[slot]);
      int64_t cap = len + len / 2 + 4096;
      hipError_t _e = hipHostMalloc(&h_blob[slot], cap);
      if (_e != hipSuccess) { if (err) *err = hipGetErrorString(_e); h_blob[slot] = nullptr; h_blob_cap[slot] = 0; return nullptr; }
      h_blob_cap[slot] = cap;
    }
    memcpy(h_blob[slot], src, len);
    return h_blob[slot];
  }
  int64_t mergebuf_cap = 0;
  bool ensure_mergebuf(int64_t m, std::string* err) {
    if (m + 1 <= mergebuf_cap) return true;
    int64_t cap = m + m / 2 + 64;
    for (void* q : {(void*)d_mdup, (void*)d_mdupx, (void*)d_mlbs})
      if (q) (void)hipFree(q);
    HIP_CHECK(hipMalloc(&d_mdup, cap * 8));
    HIP_CHECK(hipMalloc(&d_mdupx, cap * 8));
    HIP_CHECK(hipMalloc(&d_mlbs, cap * 8));
    mergebuf_cap = cap;
    return true;
  }
  uint64_t *s_a = nullptr, *s_b = nullptr, *s_c = nullptr, *s_d = nullptr,
           *s_e = nullptr;  // max_rows+2
  uint64_t *lv1 = nullptr, *lv1o = nullptr, *lv2 = nullptr, *lv2o = nullptr,
           *lv3 = nullptr, *lv3o = nullptr;

  // range/get scratch
  int max_q = 1024;
  int scan_t = 1024;            // KB_SCAN_T: threads per scan block
  int gather_gwl = 4;           // KB_GATHER_GW: log2 lanes per record group
  int gather_t = 512;           // KB_GATHER_T: threads per gather_copy block
  int gather_mode = 1;          // KB_GATHER_MODE: 1=fused record groups, 2=wave/record
  int64_t max_cap = 4352;       // winners per query cap (>= limit+1 for etcd's 500)
  int64_t arena_bytes = 384ll << 20;
  DevRangeQ* d_qs = nullptr;
  DevGetQ* d_gq = nullptr;
  // step staging block (stepstage.h): ONE device allocation whose slices are
  // the get queries, the range queries and their key tails, with a pinned
  // double-buffered mirror the bench step fills in place, so a step uploads
  // all three with one H2D. d_qs_own/d_gq_own are its max_q-sized slices,
  // the targets of the per-call uploads.
  uint8_t* d_stage = nullptr;
  int64_t stage_cap = 0;
  DevRangeQ* d_qs_own = nullptr;
  DevGetQ* d_gq_own = nullptr;
  uint8_t* h_stage[2] = {nullptr, nullptr};
  hipEvent_t ev_stage[2] = {nullptr, nullptr};
  int stage_idx = 0;
  kbstage::StepLayout stage_lay;
  int stage_nget = -1, stage_nrange = -1;  // -1: no step staged
  uint64_t* d_rows = nullptr;   // max_q*max_cap (base winners)
  uint64_t* d_rows2 = nullptr;  // delta winners
  uint64_t* d_rowsm = nullptr;  // merged winners
  int64_t* d_bounds4 = nullptr;  // [4*max_q] k_range_bounds results
  int64_t* d_offs = nullptr;    // max_q*max_cap
  int64_t *d_found = nullptr, *d_total = nullptr, *d_gbytes = nullptr;
  int32_t *d_ovf = nullptr, *d_found32 = nullptr;
  uint64_t *d_orev = nullptr, *d_ometa = nullptr;
  unsigned long long *d_scanned = nullptr, *d_bytes = nullptr;
  // pinned mirrors of the resmeta block, one per batch slot: a batch's
  // counters are read back by its own RangeBatchStart, so the next batch
  // can be queued before the host looks at them (no stream drain)
  uint8_t* h_resmeta[2] = {nullptr, nullptr};
  int64_t resmeta_bytes = 0;
  // per-slot scan start / scan end / gather end / counters-on-host events
  hipEvent_t ev_r0[2] = {nullptr, nullptr}, ev_r1[2] = {nullptr, nullptr},
             ev_r2[2] = {nullptr, nullptr}, ev_rdy[2] = {nullptr, nullptr};
  int rb_slot = 0;  // slot of the batch started last
  uint8_t* d_gbuf = nullptr;    // arena
  uint8_t* d_pack = nullptr;    // arena
  int64_t* d_goffs = nullptr;   // max_q+1
  int64_t* d_bounds = nullptr;  // compact bounds
  uint8_t* d_bkeys = nullptr;
  uint64_t* d_brevs = nullptr;

  // delta upload scratch (grown on demand)
  uint8_t* d_dkeys = nullptr;
  uint64_t *d_dmeta = nullptr, *d_drev = nullptr, *d_dvo = nullptr,
           *d_dko = nullptr;
  int64_t upload_cap = 0;

  // watcher table
  int64_t wcap = 0;
  uint8_t* d_wpfx = nullptr;
  uint32_t *d_wplen = nullptr, *d_wlive = nullptr;
  uint64_t* d_wfrom = nullptr;
  // device-resident event log ring (keys+revs; values stay host-side)
  uint8_t* er_keys = nullptr;
  uint64_t* er_rev = nullptr;
  int64_t er_cap = 0;
  uint64_t* d_bitmap = nullptr;
  int64_t bitmap_cap = 0;

  // payload ring + batched poll (all allocated lazily: PayloadArm / first
  // use). er_poff/er_plen are event-ring columns; pay is the byte ring.
  uint64_t* er_poff = nullptr;
  uint32_t* er_plen = nullptr;
  uint8_t* pay = nullptr;
  int64_t pay_cap = 0;
  uint8_t* h_pstage = nullptr;   // pinned payload staging
  int64_t h_pstage_cap = 0;
  hipEvent_t ev_w0 = nullptr, ev_w1 = nullptr, ev_w2 = nullptr;
  WpollRef *h_wrefs = nullptr, *d_wrefs = nullptr;   // ref table
  WpollSize *h_wsizes = nullptr, *d_wsizes = nullptr;
  uint64_t *h_woffs = nullptr, *d_woffs = nullptr;
  int64_t wrefs_cap = 0;
  uint8_t *d_warena = nullptr, *h_wreply = nullptr;
  int64_t warena_cap = 0, wreply_cap = 0;
  void free_wpoll() {
    for (void* q : {(void*)er_poff, (void*)er_plen, (void*)pay, (void*)d_wrefs,
                    (void*)d_wsizes, (void*)d_woffs, (void*)d_warena})
      if (q) (void)hipFree(q);
    for (void* q : {(void*)h_pstage, (void*)h_wrefs, (void*)h_wsizes,
                    (void*)h_woffs, (void*)h_wreply})
      if (q) (void)hipHostFree(q);
    for (hipEvent_t e : {ev_w0, ev_w1, ev_w2})
      if (e) (void)hipEventDestroy(e);
  }
  bool ensure_wrefs(int64_t nrefs, std::string* err) {
    if (nrefs <= wrefs_cap) return true;
    int64_t cap = std::max<int64_t>(1024, nrefs + nrefs / 2);
    for (void* q : {(void*)d_wrefs, (void*)d_wsizes, (void*)d_woffs})
      if (q) (void)hipFree(q);
    for (void* q : {(void*)h_wrefs, (void*)h_wsizes, (void*)h_woffs})
      if (q) (void)hipHostFree(q);
    d_wrefs = nullptr; d_wsizes = nullptr; d_woffs = nullptr;
    h_wrefs = nullptr; h_wsizes = nullptr; h_woffs = nullptr;
    wrefs_cap = 0;
    HIP_CHECK(hipMalloc(&d_wrefs, cap * sizeof(WpollRef)));
    HIP_CHECK(hipMalloc(&d_wsizes, cap * sizeof(WpollSize)));
    HIP_CHECK(hipMalloc(&d_woffs, cap * 8));
    HIP_CHECK(hipHostMalloc(&h_wrefs, cap * sizeof(WpollRef)));
    HIP_CHECK(hipHostMalloc(&h_wsizes, cap * sizeof(WpollSize)));
    HIP_CHECK(hipHostMalloc(&h_woffs, cap * 8));
    wrefs_cap = cap;
    return true;
  }

  // batched List (allocated on first use): per-query sizes, the emit plan
  // (base[max_q] | cum[max_q+1]) and the pinned reply
  ListSize *h_lsizes = nullptr, *d_lsizes = nullptr;
  uint64_t *h_lplan = nullptr, *d_lplan = nullptr;
  uint8_t* h_lreply = nullptr;
  int64_t lreply_cap = 0;
  int list_nq = 0;  // queries of the resident sized sub-batch
  hipEvent_t ev_l0 = nullptr, ev_l1 = nullptr, ev_l2 = nullptr;
  void free_list() {
    for (void* q : {(void*)d_lsizes, (void*)d_lplan})
      if (q) (void)hipFree(q);
    for (void* q : {(void*)h_lsizes, (void*)h_lplan, (void*)h_lreply})
      if (q) (void)hipHostFree(q);
    for (hipEvent_t e : {ev_l0, ev_l1, ev_l2})
      if (e) (void)hipEventDestroy(e);
  }
  bool ensure_list(std::string* err) {
    if (d_lsizes) return true;
    HIP_CHECK(hipEventCreate(&ev_l0));
    HIP_CHECK(hipEventCreate(&ev_l1));
    HIP_CHECK(hipEventCreate(&ev_l2));
    HIP_CHECK(hipHostMalloc(&h_lsizes, (int64_t)max_q * sizeof(ListSize) + 8));
    HIP_CHECK(hipHostMalloc(&h_lplan, (int64_t)(2 * max_q + 1) * 8));
    HIP_CHECK(hipMalloc(&d_lplan, (int64_t)(2 * max_q + 1) * 8));
    HIP_CHECK(hipMalloc(&d_lsizes, (int64_t)max_q * sizeof(ListSize)));
    return true;
  }

  // batched point read (allocated on first use): find results, arena
  // offsets, the {total; skipped; directory} block and its pinned mirror,
  // the pinned query upload mirror
  uint64_t *d_gtag = nullptr, *d_grev = nullptr, *d_gmeta = nullptr,
           *d_gaoff = nullptr, *d_ghdr = nullptr, *h_ghdr = nullptr;
  DevGetQ* h_getq = nullptr;
  int get_nq = 0;  // queries of the resident launch
  hipEvent_t ev_b0 = nullptr, ev_b1 = nullptr, ev_b2 = nullptr;
  void free_getb() {
    for (void* q : {(void*)d_gtag, (void*)d_grev, (void*)d_gmeta,
                    (void*)d_gaoff, (void*)d_ghdr})
      if (q) (void)hipFree(q);
    for (void* q : {(void*)h_ghdr, (void*)h_getq})
      if (q) (void)hipHostFree(q);
    for (hipEvent_t e : {ev_b0, ev_b1, ev_b2})
      if (e) (void)hipEventDestroy(e);
  }
  bool ensure_getb(std::string* err) {
    if (d_ghdr) return true;
    HIP_CHECK(hipEventCreate(&ev_b0));
    HIP_CHECK(hipEventCreate(&ev_b1));
    HIP_CHECK(hipEventCreate(&ev_b2));
    HIP_CHECK(hipHostMalloc(&h_ghdr, 16 + (int64_t)max_q * 32));
    HIP_CHECK(hipHostMalloc(&h_getq, (int64_t)max_q * sizeof(DevGetQ)));
    HIP_CHECK(hipMalloc(&d_gtag, (int64_t)max_q * 8));
    HIP_CHECK(hipMalloc(&d_grev, (int64_t)max_q * 8));
    HIP_CHECK(hipMalloc(&d_gmeta, (int64_t)max_q * 8));
    HIP_CHECK(hipMalloc(&d_gaoff, (int64_t)max_q * 8));
    HIP_CHECK(hipMalloc(&d_ghdr, 16 + (int64_t)max_q * 32));
    return true;
  }

  // batched Count (allocated on first use). Nothing here is shared with the
  // range batch: queries, key tails, bounds and the two counters
  // k_range_bounds zeroes are the call's own, so what LastRangeWire and a
  // later RangeBatchFinish read stays as it was.
  int64_t count_tile = kbcount::kDefaultTile;  // KB_COUNT_TILE
  int count_grid = 2048;                       // CUs x 8 blocks
  DevRangeQ *d_cq = nullptr, *h_cq = nullptr;
  uint8_t* d_ctails = nullptr;
  int64_t ctails_cap = 0;
  int64_t* d_cbounds = nullptr;             // [4 * max_q]
  uint64_t* d_cpfx = nullptr;               // [2 * max_q + 1]
  uint64_t *d_chdr = nullptr, *h_chdr = nullptr;  // [COUNT_HDR + max_q]
  unsigned long long* d_cctr = nullptr;     // [2] k_range_bounds' counter pair
  hipEvent_t ev_c0 = nullptr, ev_c1 = nullptr, ev_c2 = nullptr;
  void free_count() {
    for (void* q : {(void*)d_cq, (void*)d_ctails, (void*)d_cbounds,
                    (void*)d_cpfx, (void*)d_chdr, (void*)d_cctr})
      if (q) (void)hipFree(q);
    for (void* q : {(void*)h_cq, (void*)h_chdr})
      if (q) (void)hipHostFree(q);
    for (hipEvent_t e : {ev_c0, ev_c1, ev_c2})
      if (e) (void)hipEventDestroy(e);
  }
  bool ensure_count(int64_t tail_bytes, std::string* err) {
    if (!d_chdr) {
      HIP_CHECK(hipEventCreate(&ev_c0));
      HIP_CHECK(hipEventCreate(&ev_c1));
      HIP_CHECK(hipEventCreate(&ev_c2));
      HIP_CHECK(hipHostMalloc(&h_cq, (int64_t)max_q * sizeof(DevRangeQ)));
      HIP_CHECK(hipHostMalloc(&h_chdr, (int64_t)(COUNT_HDR + max_q) * 8));
      HIP_CHECK(hipMalloc(&d_cq, (int64_t)max_q * sizeof(DevRangeQ)));
      HIP_CHECK(hipMalloc(&d_cbounds, (int64_t)max_q * 4 * 8));
      HIP_CHECK(hipMalloc(&d_cpfx, (int64_t)(2 * max_q + 1) * 8));
      HIP_CHECK(hipMalloc(&d_cctr, 16));
      HIP_CHECK(hipMalloc(&d_chdr, (int64_t)(COUNT_HDR + max_q) * 8));
    }
    if (tail_bytes > ctails_cap || !d_ctails) {
      if (d_ctails) (void)hipFree(d_ctails);
      d_ctails = nullptr;
      ctails_cap = 0;
      int64_t cap = tail_bytes * 2 + 4096;
      HIP_CHECK(hipMalloc(&d_ctails, cap));
      ctails_cap = cap;
    }
    return true;
  }

  // KB_SCAN_DBG=1: per-phase wall_clock64 cycle sums from k_range_scan2
  // ([0]=bounds [1]=pass1a [2]=pass1b [3]=scatter [4]=merge [5]=block total)
  unsigned long long* d_dbg = nullptr;
  double wall_khz = 0;

  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  hipEvent_t ev_g0 = nullptr, ev_g1 = nullptr;  // async get lookup
  // d_orev | d_ometa | d_found32 are slices of one device block (d_orev is
  // its base) with this pinned mirror: one D2H brings a lookup's results.
  // The async lookup (launchGet) packs its three columns with stride nq at
  // the block's start, so that copy is nq * 20 bytes.
  uint8_t* h_getres = nullptr;
  int64_t getres_bytes = 0;
  // pinned double-buffered staging of EventRingPush (keys96 | revs)
  uint8_t* h_evpush[2] = {nullptr, nullptr};
  int64_t h_evpush_cap[2] = {0, 0};
  hipEvent_t ev_evpush[2] = {nullptr, nullptr};
  int evpush_idx = 0;

  // host staging (pinned for fast D2H)
  uint8_t* h_pack = nullptr;
  int64_t h_pack_cap = 0;
  bool ensure_hpack(int64_t need, std::string* err) {
    if (need <= h_pack_cap) return true;
    if (h_pack) (void)hipHostFree(h_pack);
    int64_t cap = need + need / 2;
    HIP_CHECK(hipHostMalloc(&h_pack, cap));
    h_pack_cap = cap;
    return true;
  }

  // pipelined payload D2H (bench d2h mode): ping-pong pack arenas; each
  // batch's payload copy runs on the copy stream and overlaps the NEXT
  // batch's kernels on the compute stream (the PCIe copy and the scan use
  // different engines). Slot reuse waits on that slot's prior copy.
  hipStream_t cstream = nullptr;
  uint8_t* d_packs[2] = {nullptr, nullptr};  // [0] aliases d_pack
  uint8_t* h_packs[2] = {nullptr, nullptr};
  int64_t h_packs_cap[2] = {0, 0};
  hipEvent_t ev_pk[2] = {nullptr, nullptr}, ev_cp[2] = {nullptr, nullptr};
  bool cp_busy[2] = {false, false};
  int pk_idx = 0;
  double* pack_ms_acc = nullptr;  // -> perf.pack_d2h_ms (set by Slab)
  Perf* perf = nullptr;           // -> Slab::perf (mergeRuns branch counters)
  bool validate_dn = false;       // KB_VALIDATE_DN: re-check async predictions
  // what the most recent RangeBatchFinish left behind (kb_test_last_range):
  // its counters stay in h_resmeta[last_res], its records in d_gbuf and, for a
  // pipelined d2h batch, in h_packs[last_slot]
  int last_nq = 0;
  int last_res = 0;  // its h_resmeta slot
  int64_t last_qcap = 0;
  bool last_pipe = false;
  int last_slot = 0;

  bool ensure_pipe(int idx, int64_t need, std::string* err) {
    if (!cstream) {
      HIP_CHECK(hipStreamCreate(&cstream));
      HIP_CHECK(hipEventCreate(&ev_pk[0]));
      HIP_CHECK(hipEventCreate(&ev_pk[1]));
      HIP_CHECK(hipEventCreate(&ev_cp[0]));
      HIP_CHECK(hipEventCreate(&ev_cp[1]));
      d_packs[0] = d_pack;
    }
    if (idx == 1 && !d_packs[1]) HIP_CHECK(hipMalloc(&d_packs[1], arena_bytes));
    if (need > h_packs_cap[idx]) {
      if (h_packs[idx]) (void)hipHostFree(h_packs[idx]);
      int64_t cap = need + need / 2;
      HIP_CHECK(hipHostMalloc(&h_packs[idx], cap));
      h_packs_cap[idx] = cap;
    }
    return true;
  }

  // wait for slot idx's in-flight copy (accumulating its event time)
  void wait_slot(int idx) {
    if (!cp_busy[idx]) return;
    (void)hipEventSynchronize(ev_cp[idx]);
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev_pk[idx], ev_cp[idx]) == hipSuccess &&
        pack_ms_acc)
      *pack_ms_acc += ms;
    cp_busy[idx] = false;
  }

  ~Impl() {
    wait_slot(0);
    wait_slot(1);
    if (d_packs[1]) (void)hipFree(d_packs[1]);
    for (int i = 0; i < 2; ++i) if (h_packs[i]) (void)hipHostFree(h_packs[i]);
    for (hipEvent_t e : {ev_pk[0], ev_pk[1], ev_cp[0], ev_cp[1]})
      if (e) (void)hipEventDestroy(e);
    if (cstream) (void)hipStreamDestroy(cstream);
    for (void* p : {(void*)A.keys, (void*)A.meta, (void*)A.rev, (void*)A.vo,
                    (void*)B.keys, (void*)B.meta, (void*)B.rev, (void*)B.vo,
                    (void*)DA.keys, (void*)DA.meta, (void*)DA.rev, (void*)DA.vo,
                    (void*)DB.keys, (void*)DB.meta, (void*)DB.rev, (void*)DB.vo,
                    (void*)d_rows2, (void*)d_rowsm,
                    (void*)heapA, (void*)heapB, (void*)s_a, (void*)s_b,
                    (void*)s_c, (void*)s_d, (void*)s_e, (void*)lv1, (void*)lv1o, (void*)lv2,
                    (void*)lv2o, (void*)lv3, (void*)lv3o,
                    (void*)d_stage,  // holds d_qs_own and d_gq_own
                    (void*)d_rows, (void*)d_offs,
                    (void*)d_found,  // base of the resmeta block
                    (void*)d_orev,
                    (void*)shadow, (void*)d_outpos, (void*)d_mdup, (void*)d_mdupx,
                    (void*)d_mlbs, (void*)d_gbuf,
                    (void*)d_pack, (void*)d_goffs, (void*)d_bounds,
                    (void*)d_bkeys, (void*)d_brevs, (void*)d_dkeys,
                    (void*)d_dmeta, (void*)d_drev, (void*)d_dvo, (void*)d_dko,
                    (void*)spillA, (void*)spillB, (void*)d_qtails_own,
                    (void*)A.ko, (void*)B.ko, (void*)DA.ko, (void*)DB.ko,
                    (void*)d_wpfx,
                    (void*)d_wplen, (void*)d_wlive, (void*)d_wfrom,
                    (void*)er_keys, (void*)er_rev, (void*)d_bitmap}) {
      if (p) (void)hipFree(p);
    }
    free_wpoll();
    free_list();
    free_getb();
    free_count();
    if (h_pack) (void)hipHostFree(h_pack);
    for (int i = 0; i < 2; ++i) {
      if (h_resmeta[i]) (void)hipHostFree(h_resmeta[i]);
      if (h_stage[i]) (void)hipHostFree(h_stage[i]);
      if (h_evpush[i]) (void)hipHostFree(h_evpush[i]);
      for (hipEvent_t e : {ev_r0[i], ev_r1[i], ev_r2[i], ev_rdy[i], ev_stage[i],
                           ev_evpush[i]})
        if (e) (void)hipEventDestroy(e);
    }
    for (int i = 0; i < 2; ++i) {
      if (h_uploads[i]) (void)hipHostFree(h_uploads[i]);
      if (ev_up[i]) (void)hipEventDestroy(ev_up[i]);
      if (h_qs[i]) (void)hipHostFree(h_qs[i]);
      if (ev_qs[i]) (void)hipEventDestroy(ev_qs[i]);
      if (h_blob[i]) (void)hipHostFree(h_blob[i]);
      if (ev_blob[i]) (void)hipEventDestroy(ev_blob[i]);
    }
    if (h_getres) (void)hipHostFree(h_getres);
    if (ev_g0) (void)hipEventDestroy(ev_g0);
    if (ev_g1) (void)hipEventDestroy(ev_g1);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (ev2) (void)hipEventDestroy(ev2);
    if (ev3) (void)hipEventDestroy(ev3);
    if (stream) (void)hipStreamDestroy(stream);
  }

  // exclusive scan of d_in[0..cnt) into d_out, total via small D2H
  bool scan(const uint64_t* d_in, uint64_t* d_out, int64_t cnt, uint64_t* total,
            std::string* err) {
    int64_t nb1 = ceil_div(cnt, 256);
    hipLaunchKernelGGL(k_block_scan, dim3((uint32_t)nb1), dim3(256), 0, stream,
                       d_in, d_out, lv1, cnt);
    if (nb1 > 1) {
      int64_t nb2 = ceil_div(nb1, 256);
      hipLaunchKernelGGL(k_block_scan, dim3((uint32_t)nb2), dim3(256), 0, stream,
                         lv1, lv1o, lv2, nb1);
      if (nb2 > 1) {
        int64_t nb3 = ceil_div(nb2, 256);
        hipLaunchKernelGGL(k_block_scan, dim3((uint32_t)nb3), dim3(256), 0,
                           stream, lv2, lv2o, lv3, nb2);
        if (nb3 > 1) {
          // 4th level covers up to 256^4 = 4.3G rows (nb3 <= 256 by max_rows)
          if (nb3 > 256) { if (err) *err = "scan: size too large"; return false; }
          hipLaunchKernelGGL(k_block_scan, dim3(1), dim3(256), 0, stream, lv3,
                             lv3o, lv3 + 256, nb3);
          hipLaunchKernelGGL(k_add_offsets, dim3((uint32_t)nb3), dim3(256), 0,
                             stream, lv2o, lv3o, nb2);
        }
        hipLaunchKernelGGL(k_add_offsets, dim3((uint32_t)nb2), dim3(256), 0,
                           stream, lv1o, lv2o, nb1);
      }
      hipLaunchKernelGGL(k_add_offsets, dim3((uint32_t)nb1), dim3(256), 0,
                         stream, d_out, lv1o, cnt);
    }
    if (total) {
      uint64_t last_out = 0, last_in = 0;
      HIP_CHECK(hipMemcpyAsync(&last_out, d_out + (cnt - 1), 8,
                               hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipMemcpyAsync(&last_in, const_cast<uint64_t*>(d_in) + (cnt - 1),
                               8, hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipStreamSynchronize(stream));
      *total = last_out + last_in;
    }
    return true;
  }

  bool ensure_delta(int64_t m, std::string* err) {
    if (m <= upload_cap) return true;
    int64_t cap = m + m / 2 + 1024;
    // one device block + one pinned mirror: per-step uploads become a single
    // host memcpy + ONE async H2D (five pageable copies each stalled the
    // host on the staging pool)
    if (d_dkeys) (void)hipFree(d_dkeys);
    for (int i = 0; i < 2; ++i) {
      if (h_uploads[i]) (void)hipHostFree(h_uploads[i]);
      HIP_CHECK(hipHostMalloc(&h_uploads[i], cap * (KEYW + 32)));
      if (!ev_up[i]) HIP_CHECK(hipEventCreate(&ev_up[i]));
    }
    int64_t bytes = cap * (KEYW + 32);
    HIP_CHECK(hipMalloc(&d_dkeys, bytes));
    d_dmeta = (uint64_t*)(d_dkeys + cap * KEYW);
    d_drev = d_dmeta + cap;
    d_dvo = d_drev + cap;
    d_dko = d_dvo + cap;
    upload_cap = cap;
    return true;
  }

  // generic two-run merge: src (n rows) + newer (m rows, device arrays,
  // rev-rows replace) -> dst; recomputes same_next. dst must hold n+m rows.
  bool mergeRuns(const Col& src, int64_t n, const Run& dnew,
                 int64_t m, Col& dst, int64_t* out_n, std::string* err,
                 bool device_newn_ok = false) {
    if (n + m <= 2048) {  // single-launch path only where one CU wins
      perf->merge_small++;
      hipLaunchKernelGGL(k_merge_small, dim3(1), dim3(256), 0, stream,
                         src.run(), n, dnew, m, spillA,
                         dst.keys, dst.meta, dst.rev, dst.vo, dst.ko,
                         (int64_t*)s_d);
      if (device_newn_ok) return true;  // caller knows new_n; stay async
      int64_t nn = 0;
      HIP_CHECK(hipMemcpyAsync(&nn, s_d, 8, hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipStreamSynchronize(stream));
      *out_n = nn;
      return true;
    }
    if (m > 0 && m <= 1024 && n > 0) {
      // inverted small-insert path (the per-step txn merge): m searches into
      // the n-row run, not n searches into the m new rows; rank, scatter,
      // fixup — three launches, no scratch beyond 3 x 1024 entries
      perf->merge_insert++;
      static_assert(kbmerge::kMaxNew == 1024, "small-insert bound");
      if (!d_outpos) HIP_CHECK(hipMalloc(&d_outpos, 1024 * (8 + 8 + 4)));
      int64_t* d_lbs = (int64_t*)(d_outpos + 1024);
      uint32_t* d_dups = (uint32_t*)(d_outpos + 2048);
      hipLaunchKernelGGL(k_delta_rank, dim3((uint32_t)ceil_div(m, 4)),
                         dim3(256), 0, stream, src.run(), n, dnew, m, spillA,
                         d_lbs, d_dups);
      hipLaunchKernelGGL(k_delta_scatter,
                         dim3((uint32_t)ceil_div(n + m, 256)), dim3(256), 0,
                         stream, src.run(), n, dnew, m, d_lbs, d_dups, d_outpos,
                         dst.keys, dst.meta, dst.rev, dst.vo, dst.ko,
                         (int64_t*)s_d);
      int64_t new_n;
      if (device_newn_ok) {
        new_n = *out_n;
      } else {
        new_n = 0;
        HIP_CHECK(hipMemcpyAsync(&new_n, s_d, 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
      }
      hipLaunchKernelGGL(k_same_next_fixup, dim3((uint32_t)ceil_div(2 * m, 256)),
                         dim3(256), 0, stream, dst.keys, dst.meta, dst.ko,
                         spillA, new_n, d_outpos, m);
      *out_n = new_n;
      return true;
    }
    if (n > 0 && m > 0) {
      // big inverted path (folds, bulk appends): m*log2(n) probes + two
      // prefix sums + streaming scatters (the forward n*log2(m) rank path
      // paid ~400M random probes for a 20.7M x 512k fold and is gone).
      perf->merge_big++;
      if (!ensure_mergebuf(m, err)) return false;
      HIP_CHECK(hipMemsetAsync(s_a, 0, (n + 2) * 8, stream));
      HIP_CHECK(hipMemsetAsync(s_b, 0, n * 8, stream));
      HIP_CHECK(hipMemsetAsync(d_mdup, 0, (m + 1) * 8, stream));
      hipLaunchKernelGGL(k_merge_rank_inv_big, dim3((uint32_t)ceil_div(m, 256)),
                         dim3(256), 0, stream, src.run(), n, dnew, m, spillA,
                         s_a, s_b, d_mdup, d_mlbs);
      if (!scan(d_mdup, d_mdupx, m + 1, nullptr, err)) return false;
      if (!scan(s_a, s_c, n + 2, nullptr, err)) return false;
      hipLaunchKernelGGL(k_merge_scatter_delta2, dim3((uint32_t)ceil_div(m, 256)),
                         dim3(256), 0, stream, dnew, m, d_mdupx, d_mlbs,
                         dst.keys, dst.meta, dst.rev, dst.vo, dst.ko);
      hipLaunchKernelGGL(k_merge_scatter_base2, dim3((uint32_t)ceil_div(n, 256)),
                         dim3(256), 0, stream, src.run(), s_c, s_b, dst.keys,
                         dst.meta, dst.rev, dst.vo, dst.ko, n);
      hipLaunchKernelGGL(k_set_newn, dim3(1), dim3(64), 0, stream, d_mdupx, n,
                         m, (int64_t*)s_d);
      int64_t new_n;
      if (device_newn_ok) {
        new_n = *out_n;
      } else {
        new_n = 0;
        HIP_CHECK(hipMemcpyAsync(&new_n, s_d, 8, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
      }
      hipLaunchKernelGGL(k_same_next_fixup, dim3((uint32_t)ceil_div(2 * m, 256)),
                         dim3(256), 0, stream, dst.keys, dst.meta, dst.ko,
                         spillA, new_n, d_mlbs, m);
      *out_n = new_n;
      return true;
    }
    // n == 0 here (every caller guards m > 0; n > 0 took the inverted path)
    perf->merge_empty++;
    HIP_CHECK(hipMemsetAsync(s_c, 0, 8, stream));
    if (m > 0) {
      int64_t mb = ceil_div(m, 256);
      hipLaunchKernelGGL(k_merge_scatter_delta, dim3((uint32_t)mb), dim3(256),
                         0, stream, src.run(), n, dnew, m, spillA,
                         s_c, dst.keys, dst.meta, dst.rev, dst.vo, dst.ko);
    }
    // new_n on device (s_d[0]) to avoid an extra host round trip; same_next
    // must cover the full possible extent (n+m), which is safe: rows beyond
    // new_n are untouched dst scratch read-only here... they ARE read, so
    // clamp instead: compute new_n first, then same_next sized by it.
    hipLaunchKernelGGL(k_merge_newn, dim3(1), dim3(64), 0, stream, s_c, n, m,
                       (int64_t*)s_d);
    int64_t new_n;
    if (device_newn_ok) {
      // caller tracks new_n exactly; same_next sized by the upper bound is
      // safe only if it matches — use the caller-known count via *out_n
      new_n = *out_n;
    } else {
      new_n = 0;
      HIP_CHECK(hipMemcpyAsync(&new_n, s_d, 8, hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipStreamSynchronize(stream));
    }
    if (new_n > 0) {
      int64_t sb = ceil_div(new_n, 256);
      hipLaunchKernelGGL(k_same_next, dim3((uint32_t)sb), dim3(256), 0, stream,
                         dst.keys, dst.meta, dst.ko, spillA, new_n);
    }
    *out_n = new_n;
    return true;
  }
};

static int64_t env_i64(const char* name, int64_t dflt) {
  const char* v = getenv(name);
  return v && *v ? atoll(v) : dflt;
}

static int kb_trace() { static int t = env_i64("KB_TRACE", 0) ? 1 : 0; return t; }

Slab* Slab::Create(int64_t max_rows, int64_t heap_cap, int device,
                   std::string* err) {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt == 0) {
    if (err) *err = "no HIP device (KB_ENOGPU): the product path has no CPU fallback";
    return nullptr;
  }
  if (device >= 0) HIP_CHECK_NULL(hipSetDevice(device));
  Slab* s = new Slab();
  s->p = new Impl();
  Impl* I = s->p;
  I->perf = &s->perf;
  I->validate_dn = env_i64("KB_VALIDATE_DN", 0) != 0;
  I->device = device < 0 ? 0 : device;
  I->max_rows = max_rows;
  I->heap_cap = heap_cap;
  I->max_q = (int)env_i64("KB_MAX_Q", 1024);
  I->scan_t = (int)env_i64("KB_SCAN_T", 1024);
  I->gather_t = (int)env_i64("KB_GATHER_T", 512);
  I->gather_mode = (int)env_i64("KB_GATHER_MODE", 1);
  if (I->gather_t < 64) I->gather_t = 64;
  if (I->gather_t > 1024) I->gather_t = 1024;
  I->gather_t &= ~63;
  {
    int64_t gwv = env_i64("KB_GATHER_GW", 16);
    int l = 0;
    while ((1 << l) < gwv && l < 6) ++l;
    I->gather_gwl = l;
  }
  // the scan prologue resolves 4 bounds with waves 0-3: >= 256 threads
  if (I->scan_t < 256) I->scan_t = 256;
  if (I->scan_t > 1024) I->scan_t = 1024;
  I->scan_t &= ~63;
  I->max_cap = env_i64("KB_MAX_CAP", 4352);
  I->arena_bytes = env_i64("KB_ARENA_BYTES", 384ll << 20);
  I->count_tile = kbcount::ClampTile(env_i64("KB_COUNT_TILE", kbcount::kDefaultTile));
  {
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                I->device);
    I->count_grid = (cus > 0 ? cus : 256) * 8;
  }
  std::string lerr;
  if (!err) err = &lerr;
  auto fail = [&](const char*) { delete s; return (Slab*)nullptr; };
  HIP_CHECK_NULL(hipStreamCreate(&I->stream));
  HIP_CHECK_NULL(hipEventCreate(&I->ev0));
  HIP_CHECK_NULL(hipEventCreate(&I->ev1));
  HIP_CHECK_NULL(hipEventCreate(&I->ev2));
  HIP_CHECK_NULL(hipEventCreate(&I->ev3));
  HIP_CHECK_NULL(hipEventCreate(&I->ev_g0));
  HIP_CHECK_NULL(hipEventCreate(&I->ev_g1));
  for (Impl::Col* c : {&I->A, &I->B}) {
    HIP_CHECK_NULL(hipMalloc(&c->keys, max_rows * KEYW));
    HIP_CHECK_NULL(hipMalloc(&c->meta, max_rows * 8));
    HIP_CHECK_NULL(hipMalloc(&c->rev, max_rows * 8));
    HIP_CHECK_NULL(hipMalloc(&c->vo, max_rows * 8));
    HIP_CHECK_NULL(hipMalloc(&c->ko, max_rows * 8));
  }
  if (env_i64("KB_SCAN_DBG", 0)) {
    HIP_CHECK_NULL(hipMalloc(&I->d_dbg, 8 * 8));
    HIP_CHECK_NULL(hipMemset(I->d_dbg, 0, 8 * 8));
    int khz = 0;
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, I->device);
    I->wall_khz = khz > 0 ? (double)khz : 100000.0;
  }
  I->spill_cap = env_i64("KB_SPILL_BYTES", 256ll << 20);
  HIP_CHECK_NULL(hipMalloc(&I->spillA, I->spill_cap));
  HIP_CHECK_NULL(hipMalloc(&I->spillB, I->spill_cap));
  I->delta_cap = env_i64("KB_DELTA_CAP", 1 << 16);
  if (I->delta_cap > max_rows) I->delta_cap = max_rows;
  for (Impl::Col* c : {&I->DA, &I->DB}) {
    HIP_CHECK_NULL(hipMalloc(&c->keys, I->delta_cap * KEYW));
    HIP_CHECK_NULL(hipMalloc(&c->meta, I->delta_cap * 8));
    HIP_CHECK_NULL(hipMalloc(&c->rev, I->delta_cap * 8));
    HIP_CHECK_NULL(hipMalloc(&c->vo, I->delta_cap * 8));
    HIP_CHECK_NULL(hipMalloc(&c->ko, I->delta_cap * 8));
  }
  HIP_CHECK_NULL(hipMalloc(&I->heapA, heap_cap));
  HIP_CHECK_NULL(hipMalloc(&I->heapB, heap_cap));
  HIP_CHECK_NULL(hipMalloc(&I->s_a, (max_rows + 2) * 8));
  HIP_CHECK_NULL(hipMalloc(&I->s_b, (max_rows + 2) * 8));
  HIP_CHECK_NULL(hipMalloc(&I->s_c, (max_rows + 2) * 8));
  HIP_CHECK_NULL(hipMalloc(&I->s_d, (max_rows + 2) * 8));
  HIP_CHECK_NULL(hipMalloc(&I->s_e, (max_rows + 2) * 8));
  int64_t nb1 = ceil_div(max_rows + 2, 256) + 1;
  int64_t nb2 = ceil_div(nb1, 256) + 1;
  HIP_CHECK_NULL(hipMalloc(&I->lv1, nb1 * 8));
  HIP_CHECK_NULL(hipMalloc(&I->lv1o, nb1 * 8));
  HIP_CHECK_NULL(hipMalloc(&I->lv2, nb2 * 8));
  HIP_CHECK_NULL(hipMalloc(&I->lv2o, nb2 * 8));
  HIP_CHECK_NULL(hipMalloc(&I->lv3, 512 * 8));  // +256 spill slot for level 4
  HIP_CHECK_NULL(hipMalloc(&I->lv3o, 256 * 8));
  {
    // step staging block: get queries | range queries | key tails
    I->stage_cap = kbstage::StepCapacity(I->max_q, sizeof(DevGetQ),
                                         sizeof(DevRangeQ),
                                         env_i64("KB_STAGE_TAIL_BYTES", 256 << 10));
    HIP_CHECK_NULL(hipMalloc(&I->d_stage, I->stage_cap));
    I->d_gq_own = (DevGetQ*)I->d_stage;
    I->d_qs_own = (DevRangeQ*)(I->d_stage +
                               kbstage::align_up((int64_t)I->max_q * sizeof(DevGetQ)));
    I->d_gq = I->d_gq_own;
    I->d_qs = I->d_qs_own;
    for (int i = 0; i < 2; ++i) {
      HIP_CHECK_NULL(hipHostMalloc(&I->h_stage[i], I->stage_cap));
      HIP_CHECK_NULL(hipEventCreate(&I->ev_stage[i]));
    }
  }
  HIP_CHECK_NULL(hipMalloc(&I->d_rows, (int64_t)I->max_q * I->max_cap * 8));
  HIP_CHECK_NULL(hipMalloc(&I->d_rows2, (int64_t)I->max_q * I->max_cap * 8));
  HIP_CHECK_NULL(hipMalloc(&I->d_rowsm, (int64_t)I->max_q * I->max_cap * 8));
  HIP_CHECK_NULL(hipMalloc(&I->d_bounds4, (int64_t)I->max_q * 4 * 8));
  HIP_CHECK_NULL(hipMalloc(&I->shadow, max_rows * 8));
  HIP_CHECK_NULL(hipMemset(I->shadow, 0xFF, max_rows * 8));
  HIP_CHECK_NULL(hipMalloc(&I->d_offs, (int64_t)I->max_q * I->max_cap * 8));
  {
    // found/total/gbytes/ovf/scanned/bytes live in ONE allocation so
    // RangeBatchFinish reads them all back in ONE D2H (6 small copies cost
    // ~20 us/step of copy-queue time otherwise)
    uint8_t* base = nullptr;
    I->resmeta_bytes = I->max_q * 8 * 3 + I->max_q * 4 + 16;
    HIP_CHECK_NULL(hipMalloc(&base, I->resmeta_bytes));
    I->d_found = (int64_t*)base;
    I->d_total = (int64_t*)(base + I->max_q * 8);
    I->d_gbytes = (int64_t*)(base + I->max_q * 16);
    I->d_ovf = (int32_t*)(base + I->max_q * 24);
    I->d_scanned = (unsigned long long*)(base + I->max_q * 24 + I->max_q * 4);
    I->d_bytes = I->d_scanned + 1;
    for (int i = 0; i < 2; ++i) {
      HIP_CHECK_NULL(hipHostMalloc(&I->h_resmeta[i], I->resmeta_bytes));
      memset(I->h_resmeta[i], 0, I->resmeta_bytes);
      HIP_CHECK_NULL(hipEventCreate(&I->ev_r0[i]));
      HIP_CHECK_NULL(hipEventCreate(&I->ev_r1[i]));
      HIP_CHECK_NULL(hipEventCreate(&I->ev_r2[i]));
      HIP_CHECK_NULL(hipEventCreate(&I->ev_rdy[i]));
    }
  }
  {
    // orev | ometa | found32 of a point lookup: one block, one pinned mirror
    uint8_t* base = nullptr;
    I->getres_bytes = (int64_t)I->max_q * 20;
    HIP_CHECK_NULL(hipMalloc(&base, I->getres_bytes));
    I->d_orev = (uint64_t*)base;
    I->d_ometa = I->d_orev + I->max_q;
    I->d_found32 = (int32_t*)(I->d_ometa + I->max_q);
    HIP_CHECK_NULL(hipHostMalloc(&I->h_getres, I->getres_bytes));
  }
  HIP_CHECK_NULL(hipMalloc(&I->d_gbuf, I->arena_bytes));
  HIP_CHECK_NULL(hipMalloc(&I->d_pack, I->arena_bytes));
  HIP_CHECK_NULL(hipMalloc(&I->d_goffs, (I->max_q + 1) * 8));
  HIP_CHECK_NULL(hipMalloc(&I->d_bounds, 256 * 8));
  HIP_CHECK_NULL(hipMalloc(&I->d_bkeys, 256 * KEYW));
  HIP_CHECK_NULL(hipMalloc(&I->d_brevs, 256 * 8));
  (void)fail;
  return s;
}

Slab::~Slab() { delete p; }
int64_t Slab::rows() const { return p->n; }
int64_t Slab::delta_rows() const { return p->dn; }
int64_t Slab::delta_capacity() const { return p->delta_cap; }
int64_t Slab::heap_used() const { return p->heap_used_; }
int64_t Slab::max_winner_cap() const { return p->max_cap; }

int64_t Slab::spill_used() const { return p->spill_used_; }

bool Slab::SpillAppend(const void* src, int64_t len, int64_t* off,
                       std::string* err) {
  Impl* I = p;
  if (len == 0) { *off = I->spill_used_; return true; }
  if (I->spill_used_ + len > I->spill_cap) {
    if (err) *err = "key-spill heap full (KB_SPILL_BYTES)";
    return false;
  }
  if (len > (8 << 20)) {
    HIP_CHECK(hipMemcpyAsync(I->spillA + I->spill_used_, src, len,
                             hipMemcpyHostToDevice, I->stream));
    HIP_CHECK(hipStreamSynchronize(I->stream));
    *off = I->spill_used_;
    I->spill_used_ += len;
    return true;
  }
  uint8_t* h = I->stage_blob(src, len, err);
  if (!h) return false;
  HIP_CHECK(hipMemcpyAsync(I->spillA + I->spill_used_, h, len,
                           hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_blob[I->blob_idx], I->stream));
  *off = I->spill_used_;
  I->spill_used_ += len;
  return true;
}

// Appends go to heapA/spillA only. heapB/spillB are Compact's destination:
// k_heap_scatter/k_spill_scatter write every surviving record into them from
// the A side and nothing reads them before that, so mirroring each append
// into them only doubled the bytes crossing the host link.
bool Slab::HeapAppend(const void* src, int64_t len, int64_t* off, std::string* err) {
  Impl* I = p;
  if (len == 0) { *off = I->heap_used_; return true; }
  if (I->heap_used_ + len > I->heap_cap) {
    if (err) *err = "heap full (KB_HEAP_BYTES)";
    return false;
  }
  if (len > (8 << 20)) {  // bulk loads: pageable copy + sync beats GB-scale pinned staging
    HIP_CHECK(hipMemcpyAsync(I->heapA + I->heap_used_, src, len,
                             hipMemcpyHostToDevice, I->stream));
    HIP_CHECK(hipStreamSynchronize(I->stream));
    *off = I->heap_used_;
    I->heap_used_ += len;
    return true;
  }
  uint8_t* h = I->stage_blob(src, len, err);
  if (!h) return false;
  HIP_CHECK(hipMemcpyAsync(I->heapA + I->heap_used_, h, len,
                           hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_blob[I->blob_idx], I->stream));
  *off = I->heap_used_;
  I->heap_used_ += len;
  return true;
}

bool Slab::AppendRows(const uint8_t* keys, const uint64_t* meta,
                      const uint64_t* rev, const uint64_t* vo,
                      const uint64_t* ko, int64_t m,
                      std::string* err, int64_t known_new_dn) {
  if (m == 0) return true;
  RowUpload u;
  if (!BeginRowUpload(m, &u, err)) return false;
  memcpy(u.keys, keys, m * KEYW);
  memcpy(u.meta, meta, m * 8);
  memcpy(u.rev, rev, m * 8);
  memcpy(u.vo, vo, m * 8);
  memcpy(u.ko, ko, m * 8);
  return CommitRowUpload(m, err, known_new_dn);
}

bool Slab::BeginRowUpload(int64_t m, RowUpload* u, std::string* err) {
  Impl* I = p;
  kbstage::RowLayout l;
  if (m > I->delta_cap) { if (err) *err = "append larger than delta cap"; return false; }
  if (!I->ensure_delta(m, err)) return false;
  if (!kbstage::PlanRows(m, I->upload_cap, KEYW, &l)) {
    if (err) *err = "row upload: bad row count";
    return false;
  }
  // double-buffered pinned mirror: wait only for THIS slot's previous
  // upload (two steps back — long since done), never the whole stream
  int slot = I->up_idx ^= 1;
  HIP_CHECK(hipEventSynchronize(I->ev_up[slot]));
  uint8_t* h = I->h_uploads[slot];
  u->keys = h + l.off_keys;
  u->meta = (uint64_t*)(h + l.off_meta);
  u->rev = (uint64_t*)(h + l.off_rev);
  u->vo = (uint64_t*)(h + l.off_vo);
  u->ko = (uint64_t*)(h + l.off_ko);
  return true;
}

bool Slab::CommitRowUpload(int64_t m, std::string* err, int64_t known_new_dn) {
  Impl* I = p;
  if (m == 0) return true;
  kbstage::RowLayout l;
  if (!kbstage::PlanRows(m, I->upload_cap, KEYW, &l)) {
    if (err) *err = "row upload: commit without begin";
    return false;
  }
  if (I->dn + m > I->delta_cap) {
    // fold first to make room (prediction no longer valid: go sync)
    if (!Fold(err)) return false;
    known_new_dn = -1;
  }
  bool async = known_new_dn >= 0 && !I->validate_dn;
  if (!async) HIP_CHECK(hipEventRecord(I->ev0, I->stream));
  {
    // the columns lie with stride m in the mirror and in the device block:
    // one contiguous span, ONE H2D; pinned source => a truly async enqueue
    int slot = I->up_idx;
    HIP_CHECK(hipMemcpyAsync(I->d_dkeys, I->h_uploads[slot], l.total,
                             hipMemcpyHostToDevice, I->stream));
    HIP_CHECK(hipEventRecord(I->ev_up[slot], I->stream));
  }
  int64_t new_dn = async ? known_new_dn : 0;  // async: mergeRuns reads it
  if (kb_trace()) fprintf(stderr, "[trace] AppendRows n=%lld m=%lld async=%d\n",
                          (long long)I->dn, (long long)m, (int)async);
  Run up{I->d_dkeys, (uint64_t*)(I->d_dkeys + l.off_meta),
         (uint64_t*)(I->d_dkeys + l.off_rev), (uint64_t*)(I->d_dkeys + l.off_vo),
         (uint64_t*)(I->d_dkeys + l.off_ko)};
  // shadow-mark the base rows of every inserted key BEFORE the merge
  // kernels queue (same stream => ordering is irrelevant, both read only
  // the base run and the upload)
  if (I->n > 0)
    hipLaunchKernelGGL(k_shadow_mark, dim3((uint32_t)ceil_div(m, 4)),
                       dim3(256), 0, I->stream, I->A.run(), I->n, up, m,
                       I->spillA, I->shadow);
  if (!I->mergeRuns(I->DA, I->dn, up, m, I->DB, &new_dn, err,
                    /*device_newn_ok=*/async))
    return false;
  if (async) {
    // kernels queue on the stream; subsequent reads queue behind them
    perf.merges++;
    perf.merges_async++;
    std::swap(I->DA, I->DB);
    I->dn = known_new_dn;
    return true;
  }
  HIP_CHECK(hipEventRecord(I->ev1, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev0, I->ev1);
  perf.merge_ms += ms;
  perf.merges++;
  if (known_new_dn >= 0 && new_dn != known_new_dn) {
    if (err) *err = "delta row-count prediction mismatch: " +
                    std::to_string(known_new_dn) + " vs " + std::to_string(new_dn);
    return false;
  }
  std::swap(I->DA, I->DB);
  I->dn = new_dn;
  return true;
}

bool Slab::Fold(std::string* err) {
  Impl* I = p;
  if (I->dn == 0) return true;
  if (I->n + I->dn > I->max_rows) { if (err) *err = "slab full (KB_MAX_ROWS)"; return false; }
  HIP_CHECK(hipEventRecord(I->ev2, I->stream));
  int64_t new_n = 0;
  if (!I->mergeRuns(I->A, I->n, I->DA.run(), I->dn, I->B, &new_n, err))
    return false;
  HIP_CHECK(hipEventRecord(I->ev3, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev2, I->ev3);
  perf.merge_ms += ms;
  perf.merges++;
  perf.folds++;
  std::swap(I->A, I->B);
  I->n = new_n;
  I->dn = 0;
  // base rebuilt + delta emptied => no key has a delta row
  HIP_CHECK(hipMemsetAsync(I->shadow, 0xFF, I->n * 8, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  return true;
}

bool Slab::Merge(const DeltaRows& d, std::string* err) {
  Impl* I = p;
  if (d.m == 0 && d.heap.empty()) return true;
  if (!Fold(err)) return false;  // keep run ordering invariants
  if (I->n + d.m > I->max_rows) { if (err) *err = "slab full (KB_MAX_ROWS)"; return false; }
  if (I->heap_used_ + (int64_t)d.heap.size() > I->heap_cap) {
    if (err) *err = "heap full (KB_HEAP_BYTES)";
    return false;
  }
  HIP_CHECK(hipEventRecord(I->ev0, I->stream));
  if (!d.heap.empty()) {
    HIP_CHECK(hipMemcpyAsync(I->heapA + I->heap_used_, d.heap.data(),
                             d.heap.size(), hipMemcpyHostToDevice, I->stream));
    I->heap_used_ += (int64_t)d.heap.size();
  }
  if (d.m > 0) {
    if (!I->ensure_delta(d.m, err)) return false;
    HIP_CHECK(hipMemcpyAsync(I->d_dkeys, d.keys.data(), d.m * KEYW,
                             hipMemcpyHostToDevice, I->stream));
    HIP_CHECK(hipMemcpyAsync(I->d_dmeta, d.meta.data(), d.m * 8,
                             hipMemcpyHostToDevice, I->stream));
    HIP_CHECK(hipMemcpyAsync(I->d_drev, d.rev.data(), d.m * 8,
                             hipMemcpyHostToDevice, I->stream));
    HIP_CHECK(hipMemcpyAsync(I->d_dvo, d.vo.data(), d.m * 8,
                             hipMemcpyHostToDevice, I->stream));
    if ((int64_t)d.ko.size() == d.m) {
      HIP_CHECK(hipMemcpyAsync(I->d_dko, d.ko.data(), d.m * 8,
                               hipMemcpyHostToDevice, I->stream));
    } else {
      HIP_CHECK(hipMemsetAsync(I->d_dko, 0, d.m * 8, I->stream));
    }
    int64_t new_n = 0;
    Run up{I->d_dkeys, I->d_dmeta, I->d_drev, I->d_dvo, I->d_dko};
    if (!I->mergeRuns(I->A, I->n, up, d.m, I->B, &new_n, err))
      return false;
    std::swap(I->A, I->B);
    I->n = new_n;
    // base rebuilt, delta empty (folded above) => clear shadows
    HIP_CHECK(hipMemsetAsync(I->shadow, 0xFF, I->n * 8, I->stream));
  }
  HIP_CHECK(hipEventRecord(I->ev1, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev0, I->ev1);
  perf.merge_ms += ms;
  perf.merges++;
  return true;
}

bool Slab::RangeBatch(const std::vector<DevRangeQ>& qs, bool d2h,
                      std::vector<RangeResult>* outs, std::string* err,
                      const std::string& qtails) {
  return RangeBatchEx(qs, d2h, true, outs, err, qtails);
}

bool Slab::RangeScanStart(const std::vector<DevRangeQ>& qs, std::string* err,
                          const std::string& qtails) {
  Impl* I = p;
  int nq = (int)qs.size();
  if (kb_trace()) fprintf(stderr, "[trace] RBStart nq=%d cap0=%lld\n", nq, nq?(long long)qs[0].cap:-1);
  if (nq == 0) return true;
  if (nq > I->max_q) { if (err) *err = "too many queries per batch (KB_MAX_Q)"; return false; }
  if (!I->ensure_qtails(qtails, err)) return false;
  I->stage_nrange = -1;  // the staging block no longer holds the current batch
  {
    // pinned double-buffered query upload (a 900-query batch is ~200 KB;
    // pageable hipMemcpyAsync stalls the host on the staging pool)
    if (!I->h_qs[0]) {
      for (int i = 0; i < 2; ++i) {
        HIP_CHECK(hipHostMalloc(&I->h_qs[i], sizeof(DevRangeQ) * I->max_q));
        HIP_CHECK(hipEventCreate(&I->ev_qs[i]));
      }
    }
    int slot = I->qs_idx ^= 1;
    HIP_CHECK(hipEventSynchronize(I->ev_qs[slot]));
    memcpy(I->h_qs[slot], qs.data(), sizeof(DevRangeQ) * nq);
    HIP_CHECK(hipMemcpyAsync(I->d_qs, I->h_qs[slot], sizeof(DevRangeQ) * nq,
                             hipMemcpyHostToDevice, I->stream));
    HIP_CHECK(hipEventRecord(I->ev_qs[slot], I->stream));
  }
  return launchScan(nq, err);
}

// scan half over the current batch's queries (I->d_qs / I->d_qtails, already
// queued for upload): takes the next batch slot and records its scan events
bool Slab::launchScan(int nq, std::string* err) {
  Impl* I = p;
  const int rs = I->rb_slot ^= 1;
  HIP_CHECK(hipEventRecord(I->ev_r0[rs], I->stream));
  static_assert(sizeof(unsigned long long) == 8, "counter pair layout");
  hipLaunchKernelGGL(k_range_bounds, dim3(nq), dim3(256), 0, I->stream,
                     I->A.run(), I->n, I->DA.run(), I->dn, I->spillA,
                     I->d_qtails, I->d_qs, nq, I->d_bounds4,
                     I->d_scanned /* d_bytes == d_scanned + 1 */);
  hipLaunchKernelGGL(k_range_scan2, dim3(nq), dim3((uint32_t)I->scan_t), 0, I->stream,
                     I->A.run(), I->n, I->DA.run(), I->dn, I->spillA,
                     I->d_qtails, I->d_qs, nq,
                     I->max_cap, I->d_rows, I->d_rows2, I->d_rowsm, I->d_found,
                     I->d_total, I->d_scanned, I->d_bounds4, I->shadow,
                     I->d_dbg);
  HIP_CHECK(hipEventRecord(I->ev_r1[rs], I->stream));
  return true;
}

bool Slab::RangeBatchStart(const std::vector<DevRangeQ>& qs, std::string* err,
                           const std::string& qtails) {
  int nq = (int)qs.size();
  if (!RangeScanStart(qs, err, qtails)) return false;
  if (nq == 0) return true;
  return launchGather(qs.data(), nq, err);
}

int Slab::range_slot() const { return p->rb_slot; }

// gather half + the batch's counter read-back into its slot's pinned mirror.
// hq = the batch's queries in host memory (their caps size gather mode 2).
bool Slab::launchGather(const DevRangeQ* hq, int nq, std::string* err) {
  Impl* I = p;
  const int rs = I->rb_slot;
  int64_t qcap = I->arena_bytes / nq;
  qcap &= ~15ll;
  if (I->gather_mode == 2) {
    hipLaunchKernelGGL(k_gather, dim3(nq), dim3(256), 0, I->stream, I->A.run(),
                       I->DA.run(), I->heapA, I->d_rowsm, I->max_cap,
                       I->d_found, I->d_qs, nq, I->d_gbuf, qcap, I->d_offs,
                       I->d_gbytes, I->d_ovf, I->d_bytes);
    int64_t maxw = 0;
    for (int i = 0; i < nq; ++i) {
      int64_t qc = hq[i].cap;  // packed struct: copy, do not bind
      int64_t c = qc > 0 && qc < I->max_cap ? qc : I->max_cap;
      if (c > maxw) maxw = c;
    }
    hipLaunchKernelGGL(k_gather_copy2,
                       dim3(nq, (uint32_t)ceil_div(maxw, 4)), dim3(256), 0,
                       I->stream, I->A.run(), I->DA.run(), I->spillA, I->heapA,
                       I->d_rowsm, I->max_cap, I->d_found, I->d_qs, nq,
                       I->d_gbuf, qcap, I->d_offs, I->d_ovf);
  } else {
    // offsets, overflow, byte counters and the copy in one launch
    hipLaunchKernelGGL(k_gather_fused, dim3(nq), dim3((uint32_t)I->gather_t), 0,
                       I->stream, I->A.run(), I->DA.run(), I->spillA, I->heapA,
                       I->d_rowsm, I->max_cap, I->d_found, I->d_qs, nq,
                       I->d_gbuf, qcap, I->d_gbytes, I->d_ovf, I->d_bytes,
                       I->gather_gwl);
  }
  HIP_CHECK(hipEventRecord(I->ev_r2[rs], I->stream));
  // found/total/gbytes/ovf/scanned/bytes share one device block: one D2H
  // into this slot's pinned mirror. RangeBatchFinish waits on ev_rdy of the
  // slot alone, so a later batch may already be queued behind this one.
  HIP_CHECK(hipMemcpyAsync(I->h_resmeta[rs], I->d_found, I->resmeta_bytes,
                           hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_rdy[rs], I->stream));
  return true;
}

bool Slab::RangeBatchEx(const std::vector<DevRangeQ>& qs, bool d2h, bool parse,
                        std::vector<RangeResult>* outs, std::string* err,
                        const std::string& qtails) {
  if (!RangeBatchStart(qs, err, qtails)) return false;
  return RangeBatchFinish((int)qs.size(), d2h, parse, outs, err);
}

bool Slab::RangeBatchFinish(int nq, bool d2h, bool parse,
                            std::vector<RangeResult>* outs, std::string* err,
                            int slot) {
  Impl* I = p;
  outs->assign(nq, RangeResult());
  if (nq == 0) return true;
  const int rs = slot >= 0 ? (slot & 1) : I->rb_slot;
  if (d2h && rs != I->rb_slot) {
    if (err) *err = "range finish: d2h of a batch that is no longer the latest";
    return false;
  }
  int64_t qcap = I->arena_bytes / nq;
  qcap &= ~15ll;
  I->last_nq = nq;
  I->last_qcap = qcap;
  I->last_pipe = d2h && !parse;
  I->last_res = rs;
  // the counters were read back by the batch's own start; wait for THAT
  // copy only (never the stream: a later batch may be queued behind it)
  std::vector<int64_t> found(nq), total(nq), gbytes(nq);
  std::vector<int32_t> ovf(nq);
  unsigned long long scanned = 0, bytes = 0;
  {
    HIP_CHECK(hipEventSynchronize(I->ev_rdy[rs]));
    const uint8_t* hm = I->h_resmeta[rs];
    memcpy(found.data(), hm, nq * 8);
    memcpy(total.data(), hm + I->max_q * 8, nq * 8);
    memcpy(gbytes.data(), hm + I->max_q * 16, nq * 8);
    memcpy(ovf.data(), hm + I->max_q * 24, nq * 4);
    memcpy(&scanned, hm + I->max_q * 28, 8);
    memcpy(&bytes, hm + I->max_q * 28 + 8, 8);
    if (kb_trace()) fprintf(stderr, "[trace] RBFinish nq=%d slot=%d w0=%lld ovf0=%d\n", nq, rs, (long long)found[0], (int)ovf[0]);
  }
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_r0[rs], I->ev_r1[rs]);
  perf.scan_ms += ms;
  (void)hipEventElapsedTime(&ms, I->ev_r1[rs], I->ev_r2[rs]);
  perf.gather_ms += ms;
  if (I->d_dbg) {  // KB_SCAN_DBG: block-serial ms per phase, summed over blocks
    unsigned long long c[8] = {0};
    HIP_CHECK(hipMemcpy(c, I->d_dbg, 8 * 8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemset(I->d_dbg, 0, 8 * 8));
    perf.dbg_a += (double)c[0] / I->wall_khz;
    perf.dbg_b += (double)c[1] / I->wall_khz;
    perf.dbg_c += (double)c[2] / I->wall_khz;
    perf.dbg_d += (double)c[3] / I->wall_khz;
    perf.dbg_e += (double)c[4] / I->wall_khz;
    fprintf(stderr,
            "[scan_dbg] blocks=%llu total_ms=%.2f max_block_us=%.1f avg_block_us=%.1f\n",
            c[7], (double)c[5] / I->wall_khz,
            c[7] ? (double)c[6] / I->wall_khz * 1e3 : 0.0,
            c[7] ? (double)c[5] / c[7] / I->wall_khz * 1e3 : 0.0);
  }
  perf.scan_launches++;
  perf.gather_launches++;
  perf.rows_scanned += (int64_t)scanned;
  perf.bytes_gathered += (int64_t)bytes;
  for (int q = 0; q < nq; ++q) {
    RangeResult& r = (*outs)[q];
    r.written = found[q];
    r.total = total[q];
    r.bytes = gbytes[q];
    r.overflow = ovf[q] != 0;
    perf.winners += found[q];
  }
  if (!d2h) return true;
  std::vector<int64_t> goffs(nq + 1);
  int64_t acc = 0;
  for (int q = 0; q < nq; ++q) { goffs[q] = acc; acc += ovf[q] ? 0 : gbytes[q]; }
  goffs[nq] = acc;
  if (!parse) {
    // raw bench mode: PIPELINED pack + D2H. The payload copy runs on the
    // copy stream and overlaps the next batch's kernels; slot reuse (every
    // second batch) waits on that slot's previous copy. DrainD2H() collects
    // the tail.
    I->pack_ms_acc = &perf.pack_d2h_ms;
    int idx = I->pk_idx;
    I->pk_idx ^= 1;
    // wait first: ensure_pipe may free this slot's pinned buffer, which the
    // slot's previous copy could still be writing
    I->wait_slot(idx);
    if (!I->ensure_pipe(idx, acc, err)) return false;
    I->last_slot = idx;
    HIP_CHECK(hipMemcpyAsync(I->d_goffs, goffs.data(), (nq + 1) * 8,
                             hipMemcpyHostToDevice, I->stream));
    hipLaunchKernelGGL(k_pack, dim3(nq), dim3(256), 0, I->stream, I->d_gbuf,
                       qcap, I->d_gbytes, I->d_goffs, I->d_ovf, I->d_packs[idx],
                       nq);
    HIP_CHECK(hipEventRecord(I->ev_pk[idx], I->stream));
    HIP_CHECK(hipStreamWaitEvent(I->cstream, I->ev_pk[idx], 0));
    if (acc > 0)
      HIP_CHECK(hipMemcpyAsync(I->h_packs[idx], I->d_packs[idx], acc,
                               hipMemcpyDeviceToHost, I->cstream));
    HIP_CHECK(hipEventRecord(I->ev_cp[idx], I->cstream));
    I->cp_busy[idx] = true;
    return true;
  }
  // parse mode (List/Stream): synchronous pack + one D2H + parse
  if (kb_trace()) fprintf(stderr, "[trace] parse acc=%lld w0=%lld\n", (long long)acc, (long long)(*outs)[0].written);
  I->wait_slot(0);  // d_pack aliases pipeline slot 0
  HIP_CHECK(hipEventRecord(I->ev0, I->stream));
  HIP_CHECK(hipMemcpyAsync(I->d_goffs, goffs.data(), (nq + 1) * 8,
                           hipMemcpyHostToDevice, I->stream));
  hipLaunchKernelGGL(k_pack, dim3(nq), dim3(256), 0, I->stream, I->d_gbuf, qcap,
                     I->d_gbytes, I->d_goffs, I->d_ovf, I->d_pack, nq);
  if (!I->ensure_hpack(acc, err)) return false;
  if (acc > 0)
    HIP_CHECK(hipMemcpyAsync(I->h_pack, I->d_pack, acc,
                             hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipEventRecord(I->ev1, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  (void)hipEventElapsedTime(&ms, I->ev0, I->ev1);
  perf.pack_d2h_ms += ms;
  const uint8_t* hp_end = I->h_pack + acc;
  for (int q = 0; q < nq; ++q) {
    RangeResult& r = (*outs)[q];
    if (r.overflow) continue;
    const uint8_t* pp = I->h_pack + goffs[q];
    if (r.written < 0 || r.written > I->max_cap) {
      fprintf(stderr, "[parse_bug] q=%d written=%lld total=%lld gbytes=%lld\n",
              q, (long long)r.written, (long long)r.total, (long long)r.bytes);
      if (err) *err = "corrupt range result counters";
      return false;
    }
    r.recs.reserve(r.written);
    for (int64_t j = 0; j < r.written; ++j) {
      uint64_t rv;
      uint32_t klen, vlen;
      memcpy(&rv, pp, 8);
      memcpy(&klen, pp + 8, 4);
      memcpy(&vlen, pp + 12, 4);
      if (klen > 8192 || pp + 16 + ((klen + 15) & ~15u) + vlen > hp_end) {
        fprintf(stderr,
                "[parse_bug] q=%d j=%lld/%lld rv=%llu klen=%u vlen=%u "
                "goff=%lld acc=%lld gbytes=%lld\n",
                q, (long long)j, (long long)r.written,
                (unsigned long long)rv, klen, vlen, (long long)goffs[q],
                (long long)acc, (long long)r.bytes);
        if (err) *err = "corrupt packed record";
        return false;
      }
      RangeResult::Rec rec;
      rec.rev = rv;
      rec.key.assign((const char*)pp + 16, klen);
      rec.val.assign((const char*)pp + 16 + ((klen + 15) & ~15u), vlen);
      r.recs.push_back(std::move(rec));
      pp += 16 + ((klen + 15) & ~15u) + ((vlen + 15) & ~15u);
    }
  }
  if (kb_trace()) fprintf(stderr, "[trace] parse done\n");
  return true;
}

bool Slab::DrainD2H(std::string* err) {
  p->pack_ms_acc = &perf.pack_d2h_ms;
  p->wait_slot(0);
  p->wait_slot(1);
  return true;
}

bool Slab::LastRangeWire(int src, std::string* wire, std::string* err) {
  Impl* I = p;
  const int nq = I->last_nq;
  if (src != 0 && src != 1) { if (err) *err = "last range: bad src"; return false; }
  if (src == 1 && nq > 0 && !I->last_pipe) {
    if (err) *err = "last range: the batch ran without d2h (mode bit 1)";
    return false;
  }
  if (!DrainD2H(err)) return false;
  HIP_CHECK(hipStreamSynchronize(I->stream));
  const uint8_t* hm = I->h_resmeta[I->last_res];
  std::vector<int64_t> found(nq), total(nq), gbytes(nq), goffs(nq + 1);
  std::vector<int32_t> ovf(nq);
  if (nq > 0) {
    memcpy(found.data(), hm, nq * 8);
    memcpy(total.data(), hm + I->max_q * 8, nq * 8);
    memcpy(gbytes.data(), hm + I->max_q * 16, nq * 8);
    memcpy(ovf.data(), hm + I->max_q * 24, nq * 4);
  }
  int64_t acc = 0;
  for (int q = 0; q < nq; ++q) {
    if (!ovf[q] && (gbytes[q] < 0 || gbytes[q] > I->last_qcap)) {
      if (err) *err = "last range: corrupt byte count";
      return false;
    }
    goffs[q] = acc;
    acc += ovf[q] ? 0 : gbytes[q];
  }
  goffs[nq] = acc;
  if (src == 1 && acc > I->h_packs_cap[I->last_slot]) {
    if (err) *err = "last range: pinned buffer smaller than the batch";
    return false;
  }
  wire->assign(4 + (size_t)nq * 32 + (size_t)acc, '\0');
  uint8_t* w = (uint8_t*)&(*wire)[0];
  uint32_t nq32 = (uint32_t)nq;
  memcpy(w, &nq32, 4);
  for (int q = 0; q < nq; ++q) {
    uint8_t* e = w + 4 + (size_t)q * 32;
    int32_t o = ovf[q] ? 1 : 0, z = 0;
    memcpy(e, &found[q], 8);
    memcpy(e + 8, &total[q], 8);
    memcpy(e + 16, &gbytes[q], 8);
    memcpy(e + 24, &o, 4);
    memcpy(e + 28, &z, 4);
  }
  uint8_t* body = w + 4 + (size_t)nq * 32;
  for (int q = 0; q < nq; ++q) {
    if (ovf[q] || gbytes[q] == 0) continue;
    if (src == 1) {
      memcpy(body + goffs[q], I->h_packs[I->last_slot] + goffs[q], gbytes[q]);
    } else {
      HIP_CHECK(hipMemcpy(body + goffs[q], I->d_gbuf + (int64_t)q * I->last_qcap,
                          gbytes[q], hipMemcpyDeviceToHost));
    }
  }
  return true;
}

// ---- batched List (kb_list_batch) -----------------------------------------

int Slab::max_queries() const { return p->max_q; }
int64_t Slab::arena_bytes() const { return p->arena_bytes; }
void Slab::ForgetLastRange() { p->last_nq = 0; }

bool Slab::ListSizeBatch(const std::vector<DevRangeQ>& qs,
                         const std::string& qtails, const ListSize** sizes,
                         std::string* err) {
  Impl* I = p;
  const int nq = (int)qs.size();
  I->list_nq = 0;
  if (nq <= 0 || nq > I->max_q) {
    if (err) *err = "list batch: bad sub-batch size (KB_MAX_Q)";
    return false;
  }
  if (!I->ensure_list(err)) return false;
  // the arena stops holding gathered records once an emit round runs
  I->last_nq = 0;
  (void)hipGetLastError();  // drop stale sticky errors: check OUR launches
  if (!RangeScanStart(qs, err, qtails)) return false;
  HIP_CHECK(hipEventRecord(I->ev_l0, I->stream));
  hipLaunchKernelGGL(k_list_size, dim3(nq), dim3(256), 0, I->stream,
                     I->A.run(), I->DA.run(), I->n, I->dn, I->d_rowsm,
                     I->max_cap, I->d_found, I->d_total, I->d_qs, nq,
                     (uint64_t*)I->d_offs, I->d_lsizes);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(I->ev_l1, I->stream));
  // the one small readback: 16 B per query (+ the scan's row counter)
  HIP_CHECK(hipMemcpyAsync(I->h_lsizes, I->d_lsizes, nq * sizeof(ListSize),
                           hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipMemcpyAsync((uint8_t*)I->h_lsizes + (int64_t)I->max_q * sizeof(ListSize),
                           I->d_scanned, 8, hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_r0[I->rb_slot], I->ev_r1[I->rb_slot]);
  perf.scan_ms += ms;
  ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_l0, I->ev_l1);
  perf.list_ms += ms;
  perf.scan_launches++;
  unsigned long long scanned = 0;
  memcpy(&scanned, (uint8_t*)I->h_lsizes + (int64_t)I->max_q * sizeof(ListSize), 8);
  perf.rows_scanned += (int64_t)scanned;
  I->list_nq = nq;
  *sizes = I->h_lsizes;
  return true;
}

uint8_t* Slab::ListReply(int64_t total, std::string* err) {
  Impl* I = p;
  if (total > I->lreply_cap) {
    if (I->h_lreply) (void)hipHostFree(I->h_lreply);
    I->h_lreply = nullptr;
    I->lreply_cap = 0;
    int64_t cap = std::max<int64_t>(1 << 20, total + total / 2);
    HIP_CHECK_NULL(hipHostMalloc(&I->h_lreply, cap));
    I->lreply_cap = cap;
  }
  return I->h_lreply;
}

bool Slab::ListPlanStaging(uint64_t** base, uint64_t** cum, std::string* err) {
  Impl* I = p;
  if (!I->ensure_list(err)) return false;
  *base = I->h_lplan;
  *cum = I->h_lplan + I->max_q;
  return true;
}

bool Slab::ListEmit(int nq, int64_t span, uint8_t* reply, int64_t reply_off,
                    std::string* err) {
  Impl* I = p;
  if (!I->d_lsizes || nq <= 0 || nq != I->list_nq || span < 0 ||
      span > I->arena_bytes || reply != I->h_lreply || reply_off < 0 ||
      reply_off + span > I->lreply_cap) {
    if (err) *err = "list batch: no resident sub-batch or bad emit span";
    return false;
  }
  const uint64_t* cum = I->h_lplan + I->max_q;
  const uint64_t nrec = cum[nq];
  if (nrec > (uint64_t)nq * (uint64_t)I->max_cap) {
    if (err) *err = "list batch: emit plan names more records than the table holds";
    return false;
  }
  HIP_CHECK(hipMemcpyAsync(I->d_lplan, I->h_lplan, (int64_t)(2 * I->max_q + 1) * 8,
                           hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_l0, I->stream));
  if (nrec > 0) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_list_emit, dim3((uint32_t)ceil_div((int64_t)nrec, 4)),
                       dim3(256), 0, I->stream, I->A.run(), I->DA.run(), I->n,
                       I->dn, I->spillA, I->spill_used_, I->heapA,
                       I->heap_used_, I->d_rowsm, I->max_cap, I->d_qs, nq,
                       (const uint64_t*)I->d_offs, I->d_lplan,
                       I->d_lplan + I->max_q, I->d_gbuf, I->arena_bytes);
    HIP_CHECK(hipGetLastError());
    perf.list_emit_launches++;
  }
  HIP_CHECK(hipEventRecord(I->ev_l1, I->stream));
  if (nrec > 0 && span > 0)
    HIP_CHECK(hipMemcpyAsync(reply + reply_off, I->d_gbuf, span,
                             hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_l2, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_l0, I->ev_l1);
  perf.list_ms += ms;
  ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_l1, I->ev_l2);
  perf.list_d2h_ms += ms;
  if (nrec > 0) perf.list_batch_bytes += span;
  return true;
}

// ---- batched point read (kb_get_batch) ------------------------------------

bool Slab::GetBatchLaunch(const DevGetQ* qs, int nq, const std::string& qtails,
                          bool no_values, uint64_t committed,
                          const GetBatchHdr** hdr, std::string* err) {
  Impl* I = p;
  I->get_nq = 0;
  if (nq <= 0 || nq > I->max_q) {
    if (err) *err = "get batch: bad sub-batch size (KB_MAX_Q)";
    return false;
  }
  if (!I->ensure_getb(err)) return false;
  if (!I->ensure_qtails(qtails, err)) return false;
  // the arena stops holding gathered records once the emit runs
  I->last_nq = 0;
  memcpy(I->h_getq, qs, sizeof(DevGetQ) * (size_t)nq);
  HIP_CHECK(hipMemcpyAsync(I->d_gq, I->h_getq, sizeof(DevGetQ) * (size_t)nq,
                           hipMemcpyHostToDevice, I->stream));
  (void)hipGetLastError();  // drop stale sticky errors: check OUR launches
  HIP_CHECK(hipEventRecord(I->ev_b0, I->stream));
  hipLaunchKernelGGL(k_get_find, dim3((uint32_t)ceil_div(nq, 4)), dim3(256), 0,
                     I->stream, I->A.run(), I->DA.run(), I->n, I->dn,
                     I->spillA, I->d_qtails, I->d_gq, nq, I->d_gtag,
                     I->d_grev, I->d_gmeta);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_get_plan, dim3(1), dim3(256), 0, I->stream, I->d_gtag,
                     I->d_grev, I->d_gmeta, nq, no_values ? 1 : 0, committed,
                     I->d_gaoff, I->d_ghdr);
  HIP_CHECK(hipGetLastError());
  if (!no_values) {  // nothing to copy otherwise: every vlen is 0
    hipLaunchKernelGGL(k_get_emit, dim3((uint32_t)nq), dim3(256), 0, I->stream,
                       I->A.run(), I->DA.run(), I->n, I->dn, I->heapA,
                       I->heap_used_, I->d_gtag, I->d_gaoff, I->d_ghdr, nq,
                       I->d_gbuf, I->arena_bytes,
                       (unsigned long long*)(I->d_ghdr + 1));
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipEventRecord(I->ev_b1, I->stream));
  // the one small readback: total, skipped and 32 B per query
  HIP_CHECK(hipMemcpyAsync(I->h_ghdr, I->d_ghdr, 16 + (int64_t)nq * 32,
                           hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_b2, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_b0, I->ev_b1);
  perf.get_batch_ms += ms;
  ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_b1, I->ev_b2);
  perf.get_batch_d2h_ms += ms;
  perf.get_batch_launches++;
  I->get_nq = nq;
  *hdr = (const GetBatchHdr*)I->h_ghdr;
  return true;
}

// ---- batched Count (kb_count_batch) ---------------------------------------

int64_t Slab::count_tile() const { return p->count_tile; }

bool Slab::CountBatchLaunch(const DevRangeQ* qs, int nq,
                            const std::string& qtails,
                            const CountBatchHdr** hdr, std::string* err) {
  Impl* I = p;
  static_assert(sizeof(CountBatchHdr) == (COUNT_HDR + 1) * 8, "count header");
  if (nq <= 0 || nq > I->max_q) {
    if (err) *err = "count batch: bad sub-batch size (KB_MAX_Q)";
    return false;
  }
  if (!I->ensure_count((int64_t)qtails.size(), err)) return false;
  memcpy(I->h_cq, qs, sizeof(DevRangeQ) * (size_t)nq);
  HIP_CHECK(hipMemcpyAsync(I->d_cq, I->h_cq, sizeof(DevRangeQ) * (size_t)nq,
                           hipMemcpyHostToDevice, I->stream));
  if (!qtails.empty())
    HIP_CHECK(hipMemcpyAsync(I->d_ctails, qtails.data(), qtails.size(),
                             hipMemcpyHostToDevice, I->stream));
  (void)hipGetLastError();  // drop stale sticky errors: check OUR launches
  hipLaunchKernelGGL(k_range_bounds, dim3(nq), dim3(256), 0, I->stream,
                     I->A.run(), I->n, I->DA.run(), I->dn, I->spillA,
                     I->d_ctails, I->d_cq, nq, I->d_cbounds, I->d_cctr);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(I->ev_c0, I->stream));
  hipLaunchKernelGGL(k_count_plan, dim3(1), dim3(256), 0, I->stream,
                     I->d_cbounds, nq, I->count_tile, I->d_cpfx, I->d_chdr);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_count_tiles, dim3((uint32_t)I->count_grid), dim3(256), 0,
                     I->stream, I->A.run(), I->n, I->DA.run(), I->dn, I->shadow,
                     I->d_cq, nq, I->d_cbounds, I->d_cpfx, I->count_tile,
                     I->d_chdr);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(I->ev_c1, I->stream));
  // the one small readback: four totals and 8 B per query
  HIP_CHECK(hipMemcpyAsync(I->h_chdr, I->d_chdr, (int64_t)(COUNT_HDR + nq) * 8,
                           hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_c2, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_c0, I->ev_c1);
  perf.count_ms += ms;
  ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_c1, I->ev_c2);
  perf.count_d2h_ms += ms;
  const CountBatchHdr* h = (const CountBatchHdr*)I->h_chdr;
  if (h->tiles != h->tiles_planned || h->rows != h->rows_planned) {
    if (err) *err = "count batch: the tile kernel did not cover the plan";
    return false;
  }
  perf.count_batch_launches++;
  perf.count_batch_tiles += (int64_t)h->tiles;
  perf.count_batch_rows += (int64_t)h->rows;
  *hdr = h;
  return true;
}

bool Slab::GetBatchFetch(int64_t span, uint8_t* reply, int64_t reply_off,
                         std::string* err) {
  Impl* I = p;
  if (I->get_nq <= 0 || span <= 0 || span > I->arena_bytes ||
      reply != I->h_lreply || reply_off < 0 ||
      reply_off + span > I->lreply_cap) {
    if (err) *err = "get batch: no resident launch or bad value span";
    return false;
  }
  HIP_CHECK(hipEventRecord(I->ev_b1, I->stream));
  HIP_CHECK(hipMemcpyAsync(reply + reply_off, I->d_gbuf, span,
                           hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_b2, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_b1, I->ev_b2);
  perf.get_batch_d2h_ms += ms;
  perf.get_batch_bytes += span;
  return true;
}

bool Slab::GetBatchHostValue(const DevGetQ& q, const std::string& qtails,
                             uint64_t mod_rev, uint64_t vlen, uint8_t* dst,
                             std::string* err) {
  Impl* I = p;
  I->get_nq = 0;  // the find results of the resident launch are overwritten
  if (!I->ensure_getb(err)) return false;
  if (!I->ensure_qtails(qtails, err)) return false;
  memcpy(I->h_getq, &q, sizeof(DevGetQ));
  HIP_CHECK(hipMemcpyAsync(I->d_gq, I->h_getq, sizeof(DevGetQ),
                           hipMemcpyHostToDevice, I->stream));
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_get_find, dim3(1), dim3(256), 0, I->stream, I->A.run(),
                     I->DA.run(), I->n, I->dn, I->spillA, I->d_qtails, I->d_gq,
                     1, I->d_gtag, I->d_grev, I->d_gmeta);
  HIP_CHECK(hipGetLastError());
  uint64_t* h = I->h_ghdr;  // pinned scratch: tag | rev | meta | vo
  HIP_CHECK(hipMemcpyAsync(h, I->d_gtag, 8, hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipMemcpyAsync(h + 1, I->d_grev, 8, hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipMemcpyAsync(h + 2, I->d_gmeta, 8, hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  const uint64_t tag = h[0];
  const bool isd = (tag & ROW_TAG_DELTA) != 0;
  const int64_t row = (int64_t)(tag & ROW_MASK);
  if (tag == GET_ROW_NONE || row >= (isd ? I->dn : I->n) || h[1] != mod_rev ||
      (h[2] & M_TOMB) || meta_vlen(h[2]) != vlen) {
    if (err) *err = "get batch: a host-path query changed under the mutex";
    return false;
  }
  HIP_CHECK(hipMemcpyAsync(h + 3, (isd ? I->DA.vo : I->A.vo) + row, 8,
                           hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  const uint64_t vo = h[3];
  if (vo > (uint64_t)I->heap_used_ || vlen > (uint64_t)I->heap_used_ - vo) {
    if (err) *err = "get batch: a host-path value lies outside the heap";
    return false;
  }
  HIP_CHECK(hipEventRecord(I->ev_b1, I->stream));
  HIP_CHECK(hipMemcpyAsync(dst, I->heapA + vo, vlen, hipMemcpyDeviceToHost,
                           I->stream));
  HIP_CHECK(hipEventRecord(I->ev_b2, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_b1, I->ev_b2);
  perf.get_batch_d2h_ms += ms;
  return true;
}

bool Slab::GetBatch(const std::vector<DevGetQ>& qs, std::vector<GetResult>* outs,
                    std::string* err, const std::string& qtails) {
  return GetBatchEx(qs, true, outs, err, qtails);
}

bool Slab::GetBatchStart(const std::vector<DevGetQ>& qs, std::string* err,
                         const std::string& qtails) {
  Impl* I = p;
  int nq = (int)qs.size();
  if (nq == 0) return true;
  if (nq > I->max_q) { if (err) *err = "too many gets per batch"; return false; }
  if (!I->ensure_qtails(qtails, err)) return false;
  I->stage_nget = -1;  // the staging block no longer holds the current batch
  HIP_CHECK(hipMemcpyAsync(I->d_gq, qs.data(), sizeof(DevGetQ) * nq,
                           hipMemcpyHostToDevice, I->stream));
  return launchGet(nq, err);
}

// meta-only lookup over the current batch's get queries (I->d_gq /
// I->d_qtails) + ONE D2H of the orev|ometa|found32 block
bool Slab::launchGet(int nq, std::string* err) {
  Impl* I = p;
  HIP_CHECK(hipEventRecord(I->ev_g0, I->stream));
  int blocks = (int)ceil_div(nq, 4);
  hipLaunchKernelGGL(k_get2, dim3(blocks), dim3(256), 0, I->stream,
                     I->A.run(), I->DA.run(), I->n, I->dn, I->spillA,
                     I->d_qtails, I->heapA, I->d_gq, nq, 0,
                     I->d_gbuf, 0, I->d_orev, I->d_orev + nq,
                     (int32_t*)(I->d_orev + 2 * nq), I->d_ovf);
  // the three result columns lie with stride nq in the block (GetBatchFinish
  // reads them so): the read-back is the nq * 20 bytes of this lookup
  HIP_CHECK(hipMemcpyAsync(I->h_getres, I->d_orev, (int64_t)nq * 20,
                           hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_g1, I->stream));
  return true;
}

// ---- step staging block (bench step: one upload for gets, ranges, tails) --

bool Slab::StepStageBegin(int nget, int nrange, StepStage* st, std::string* err) {
  Impl* I = p;
  I->stage_nget = I->stage_nrange = -1;
  kbstage::StepLayout l;
  if (!kbstage::PlanStep(nget, nrange, I->max_q, sizeof(DevGetQ),
                         sizeof(DevRangeQ), I->stage_cap, &l)) {
    if (err) *err = "too many queries per batch (KB_MAX_Q)";
    return false;
  }
  // wait only for this slot's previous upload (two steps back)
  int slot = I->stage_idx ^= 1;
  HIP_CHECK(hipEventSynchronize(I->ev_stage[slot]));
  I->stage_lay = l;
  uint8_t* h = I->h_stage[slot];
  st->gq = (DevGetQ*)(h + l.off_getq);
  st->rq = (DevRangeQ*)(h + l.off_rangeq);
  st->tails = h + l.off_tails;
  st->tail_cap = l.tail_cap;
  I->stage_nget = nget;
  I->stage_nrange = nrange;
  return true;
}

bool Slab::StepStageCommit(int64_t tail_bytes, std::string* err) {
  Impl* I = p;
  if (I->stage_nget < 0 || I->stage_nrange < 0) {
    if (err) *err = "step stage: commit without begin";
    return false;
  }
  const kbstage::StepLayout& l = I->stage_lay;
  int64_t span = kbstage::StepSpan(l, tail_bytes);
  if (span < 0) {
    I->stage_nget = I->stage_nrange = -1;
    if (err) *err = "step stage: key tails exceed the staging block";
    return false;
  }
  int slot = I->stage_idx;
  if (span > 0) {
    HIP_CHECK(hipMemcpyAsync(I->d_stage, I->h_stage[slot], span,
                             hipMemcpyHostToDevice, I->stream));
    HIP_CHECK(hipEventRecord(I->ev_stage[slot], I->stream));
  }
  // the kernels of this step read the staged slices
  I->d_gq = (DevGetQ*)(I->d_stage + l.off_getq);
  I->d_qs = (DevRangeQ*)(I->d_stage + l.off_rangeq);
  I->d_qtails = I->d_stage + l.off_tails;
  return true;
}

bool Slab::GetBatchStartStaged(std::string* err) {
  Impl* I = p;
  if (I->stage_nget < 0) { if (err) *err = "step stage: no staged gets"; return false; }
  if (I->stage_nget == 0) return true;
  return launchGet(I->stage_nget, err);
}

bool Slab::RangeBatchStartStaged(std::string* err) {
  Impl* I = p;
  if (I->stage_nrange < 0) { if (err) *err = "step stage: no staged ranges"; return false; }
  int nq = I->stage_nrange;
  if (nq == 0) return true;
  if (!launchScan(nq, err)) return false;
  return launchGather((const DevRangeQ*)(I->h_stage[I->stage_idx] +
                                         I->stage_lay.off_rangeq), nq, err);
}

bool Slab::GetBatchFinish(int nq, std::vector<GetResult>* outs, std::string* err) {
  Impl* I = p;
  outs->assign(nq, GetResult());
  if (nq == 0) return true;
  HIP_CHECK(hipEventSynchronize(I->ev_g1));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_g0, I->ev_g1);
  perf.get_ms += ms;
  perf.get_launches++;
  const uint64_t* h_orev = (const uint64_t*)I->h_getres;
  const uint64_t* h_ometa = h_orev + nq;
  const int32_t* h_found = (const int32_t*)(h_ometa + nq);
  for (int q = 0; q < nq; ++q) {
    GetResult& g = (*outs)[q];
    g.found = h_found[q] != 0;
    if (!g.found) continue;
    uint64_t m = h_ometa[q];
    g.rev = h_orev[q];
    g.tomb = (m & M_TOMB) != 0;
    g.vlen = meta_vlen(m);
  }
  return true;
}

bool Slab::GetBatchEx(const std::vector<DevGetQ>& qs, bool values,
                      std::vector<GetResult>* outs, std::string* err,
                      const std::string& qtails) {
  Impl* I = p;
  auto tt0 = std::chrono::steady_clock::now();
  auto lap = [&](double* acc) {
    auto t = std::chrono::steady_clock::now();
    *acc += std::chrono::duration<double>(t - tt0).count() * 1e3;
    tt0 = t;
  };
  int nq = (int)qs.size();
  outs->assign(nq, GetResult());
  if (nq == 0) return true;
  if (nq > I->max_q) { if (err) *err = "too many gets per batch"; return false; }
  if (!I->ensure_qtails(qtails, err)) return false;
  int64_t slot = I->arena_bytes / nq;
  slot &= ~15ll;
  lap(&perf.dbg_a);
  HIP_CHECK(hipMemcpyAsync(I->d_gq, qs.data(), sizeof(DevGetQ) * nq,
                           hipMemcpyHostToDevice, I->stream));
  lap(&perf.dbg_b);
  HIP_CHECK(hipEventRecord(I->ev0, I->stream));
  int blocks = (int)ceil_div(nq, 4);
  hipLaunchKernelGGL(k_get2, dim3(blocks), dim3(256), 0, I->stream,
                     I->A.run(), I->DA.run(), I->n, I->dn, I->spillA,
                     I->d_qtails, I->heapA, I->d_gq, nq, values ? 1 : 0,
                     I->d_gbuf, slot, I->d_orev, I->d_ometa, I->d_found32,
                     I->d_ovf);
  HIP_CHECK(hipEventRecord(I->ev1, I->stream));
  std::vector<uint64_t> orev(nq), ometa(nq);
  std::vector<int32_t> ofound(nq), oovf(nq);
  HIP_CHECK(hipMemcpyAsync(orev.data(), I->d_orev, nq * 8, hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipMemcpyAsync(ometa.data(), I->d_ometa, nq * 8, hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipMemcpyAsync(ofound.data(), I->d_found32, nq * 4, hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipMemcpyAsync(oovf.data(), I->d_ovf, nq * 4, hipMemcpyDeviceToHost, I->stream));
  lap(&perf.dbg_c);
  HIP_CHECK(hipStreamSynchronize(I->stream));
  lap(&perf.dbg_d);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev0, I->ev1);
  perf.get_ms += ms;
  perf.get_launches++;
  for (int q = 0; q < nq; ++q) {
    GetResult& g = (*outs)[q];
    g.found = ofound[q] != 0;
    if (!g.found) continue;
    if (oovf[q]) { if (err) *err = "get value exceeds arena slot"; return false; }
    g.rev = orev[q];
    g.tomb = (ometa[q] & M_TOMB) != 0;
    uint32_t vlen = meta_vlen(ometa[q]);
    if (!values) { g.vlen = vlen; continue; }
    g.vlen = vlen;
    g.val.resize(vlen);
    if (vlen)
      HIP_CHECK(hipMemcpy(g.val.data(), I->d_gbuf + (int64_t)q * slot, vlen,
                          hipMemcpyDeviceToHost));
  }
  lap(&perf.dbg_e);
  return true;
}

bool Slab::Compact(const std::vector<std::pair<Bound, Bound>>& borders,
                   uint64_t compact_rev, const std::vector<uint64_t>& timeout_revs,
                   std::string* err) {
  if (timeout_revs.size() != borders.size()) {
    if (err) *err = "Compact: timeout_revs must be per border pair";
    return false;
  }
  Impl* I = p;
  if (!Fold(err)) return false;  // compaction sweeps the single base run
  int64_t n = I->n;
  if (n == 0) return true;
  HIP_CHECK(hipEventRecord(I->ev0, I->stream));
  // keep := 1
  hipLaunchKernelGGL(k_fill_u64, dim3((uint32_t)ceil_div(n, 256)), dim3(256), 0,
                     I->stream, I->s_a, 1ull, n);
  // resolve border row ranges
  int nb = (int)borders.size() * 2;
  if (nb > 256) { if (err) *err = "too many compact borders"; return false; }
  std::vector<uint8_t> bkeys((size_t)nb * KEYW);
  std::vector<uint64_t> brevs(nb);
  for (size_t i = 0; i < borders.size(); ++i) {
    memcpy(bkeys.data() + (2 * i) * KEYW, borders[i].first.key, KEYW);
    brevs[2 * i] = borders[i].first.rev;
    memcpy(bkeys.data() + (2 * i + 1) * KEYW, borders[i].second.key, KEYW);
    brevs[2 * i + 1] = borders[i].second.rev;
  }
  HIP_CHECK(hipMemcpyAsync(I->d_bkeys, bkeys.data(), bkeys.size(),
                           hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipMemcpyAsync(I->d_brevs, brevs.data(), nb * 8,
                           hipMemcpyHostToDevice, I->stream));
  hipLaunchKernelGGL(k_find_bounds, dim3(1), dim3(256), 0, I->stream,
                     I->A.run(), n, I->spillA, I->d_bkeys, I->d_brevs, nb,
                     I->d_bounds);
  std::vector<int64_t> hb(nb);
  HIP_CHECK(hipMemcpyAsync(hb.data(), I->d_bounds, nb * 8, hipMemcpyDeviceToHost,
                           I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  for (int i = 0; i < nb; i += 2) {
    int64_t lo = hb[i], hi = hb[i + 1];
    if (hi <= lo) continue;
    hipLaunchKernelGGL(k_compact_mark, dim3((uint32_t)ceil_div(hi - lo, 256)),
                       dim3(256), 0, I->stream, I->A.meta, I->A.rev, I->A.vo, lo,
                       hi, compact_rev, timeout_revs[i / 2], I->s_a);
  }
  // new row index
  uint64_t kept = 0;
  if (!I->scan(I->s_a, I->s_b, n, &kept, err)) return false;
  // heap offsets
  hipLaunchKernelGGL(k_heap_sizes, dim3((uint32_t)ceil_div(n, 256)), dim3(256),
                     0, I->stream, I->s_a, I->A.rev, I->A.meta, I->s_c, n);
  uint64_t new_heap = 0;
  if (!I->scan(I->s_c, I->s_d, n, &new_heap, err)) return false;
  // key-spill offsets (tails of surviving keys > KEYW)
  hipLaunchKernelGGL(k_spill_sizes, dim3((uint32_t)ceil_div(n, 256)), dim3(256),
                     0, I->stream, I->s_a, I->A.meta, I->s_c, n);
  uint64_t new_spill = 0;
  if (!I->scan(I->s_c, I->s_e, n, &new_spill, err)) return false;
  hipLaunchKernelGGL(k_compact_scatter, dim3((uint32_t)ceil_div(n, 256)),
                     dim3(256), 0, I->stream, I->A.keys, I->A.meta, I->A.rev,
                     I->A.vo, I->A.ko, I->s_a, I->s_b, I->s_d, I->s_e,
                     I->B.keys, I->B.meta, I->B.rev, I->B.vo, I->B.ko, n);
  hipLaunchKernelGGL(k_heap_scatter, dim3((uint32_t)ceil_div(n, 4)), dim3(256),
                     0, I->stream, I->s_a, I->A.rev, I->A.meta, I->A.vo, I->s_d,
                     I->heapA, I->heapB, n);
  if (new_spill > 0)
    hipLaunchKernelGGL(k_spill_scatter, dim3((uint32_t)ceil_div(n, 4)),
                       dim3(256), 0, I->stream, I->s_a, I->A.meta, I->A.ko,
                       I->s_e, I->spillA, I->spillB, n);
  int64_t sb = ceil_div((int64_t)kept, 256);
  if (kept > 0)
    hipLaunchKernelGGL(k_same_next, dim3((uint32_t)sb), dim3(256), 0, I->stream,
                       I->B.keys, I->B.meta, I->B.ko, I->spillB, (int64_t)kept);
  HIP_CHECK(hipEventRecord(I->ev1, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev0, I->ev1);
  perf.compact_ms += ms;
  perf.compacts++;
  std::swap(I->A, I->B);
  std::swap(I->heapA, I->heapB);
  std::swap(I->spillA, I->spillB);
  I->n = (int64_t)kept;
  // compaction folds the delta first and rewrites the base => clear shadows
  if (I->n > 0)
    HIP_CHECK(hipMemsetAsync(I->shadow, 0xFF, I->n * 8, I->stream));
  I->heap_used_ = (int64_t)new_heap;
  I->spill_used_ = (int64_t)new_spill;
  HIP_CHECK(hipStreamSynchronize(I->stream));
  return true;
}

bool Slab::Dump(std::vector<DumpRow>* rows_out, std::string* err) {
  Impl* I = p;
  if (!Fold(err)) return false;
  rows_out->clear();
  int64_t n = I->n;
  if (n == 0) return true;
  std::vector<uint8_t> keys((size_t)n * KEYW);
  std::vector<uint64_t> meta(n), rev(n), vo(n), ko(n);
  std::vector<uint8_t> heap(I->heap_used_);
  std::vector<uint8_t> spill(I->spill_used_);
  HIP_CHECK(hipMemcpyAsync(keys.data(), I->A.keys, keys.size(), hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipMemcpyAsync(meta.data(), I->A.meta, n * 8, hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipMemcpyAsync(rev.data(), I->A.rev, n * 8, hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipMemcpyAsync(vo.data(), I->A.vo, n * 8, hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipMemcpyAsync(ko.data(), I->A.ko, n * 8, hipMemcpyDeviceToHost, I->stream));
  if (I->heap_used_)
    HIP_CHECK(hipMemcpyAsync(heap.data(), I->heapA, I->heap_used_, hipMemcpyDeviceToHost, I->stream));
  if (I->spill_used_)
    HIP_CHECK(hipMemcpyAsync(spill.data(), I->spillA, I->spill_used_, hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  rows_out->reserve(n);
  for (int64_t i = 0; i < n; ++i) {
    DumpRow r;
    uint32_t klen = meta_klen(meta[i]);
    uint32_t kin = klen > (uint32_t)KEYW ? (uint32_t)KEYW : klen;
    r.key.assign((const char*)keys.data() + i * KEYW, kin);
    if (klen > (uint32_t)KEYW)  // spill tail (keys > 96B)
      r.key.append((const char*)spill.data() + ko[i], klen - KEYW);
    r.rev = rev[i];
    r.meta = meta[i];
    r.vo = vo[i];
    if (rev[i] > 0) r.val.assign((const char*)heap.data() + vo[i], meta_vlen(meta[i]));
    rows_out->push_back(std::move(r));
  }
  return true;
}

bool Slab::WatcherSet(int64_t slot, const uint8_t* prefix, uint32_t plen,
                      uint64_t from_rev, std::string* err) {
  Impl* I = p;
  if (slot >= I->wcap) {
    int64_t cap = std::max<int64_t>(1024, slot + slot / 2 + 1);
    uint8_t* npfx; uint32_t *nplen, *nlive; uint64_t* nfrom;
    HIP_CHECK(hipMalloc(&npfx, cap * KEYW));
    HIP_CHECK(hipMalloc(&nplen, cap * 4));
    HIP_CHECK(hipMalloc(&nlive, cap * 4));
    HIP_CHECK(hipMalloc(&nfrom, cap * 8));
    HIP_CHECK(hipMemsetAsync(nlive, 0, cap * 4, I->stream));
    if (I->wcap > 0) {
      HIP_CHECK(hipMemcpyAsync(npfx, I->d_wpfx, I->wcap * KEYW, hipMemcpyDeviceToDevice, I->stream));
      HIP_CHECK(hipMemcpyAsync(nplen, I->d_wplen, I->wcap * 4, hipMemcpyDeviceToDevice, I->stream));
      HIP_CHECK(hipMemcpyAsync(nlive, I->d_wlive, I->wcap * 4, hipMemcpyDeviceToDevice, I->stream));
      HIP_CHECK(hipMemcpyAsync(nfrom, I->d_wfrom, I->wcap * 8, hipMemcpyDeviceToDevice, I->stream));
    }
    HIP_CHECK(hipStreamSynchronize(I->stream));
    for (void* q : {(void*)I->d_wpfx, (void*)I->d_wplen, (void*)I->d_wlive, (void*)I->d_wfrom})
      if (q) (void)hipFree(q);
    I->d_wpfx = npfx; I->d_wplen = nplen; I->d_wlive = nlive; I->d_wfrom = nfrom;
    I->wcap = cap;
  }
  uint8_t buf[KEYW] = {0};
  memcpy(buf, prefix, plen > KEYW ? KEYW : plen);
  uint32_t one = 1;
  HIP_CHECK(hipMemcpyAsync(I->d_wpfx + slot * KEYW, buf, KEYW, hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipMemcpyAsync(I->d_wplen + slot, &plen, 4, hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipMemcpyAsync(I->d_wfrom + slot, &from_rev, 8, hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipMemcpyAsync(I->d_wlive + slot, &one, 4, hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  return true;
}

void Slab::WatcherClear(int64_t slot) {
  Impl* I = p;
  if (slot >= I->wcap) return;
  uint32_t zero = 0;
  (void)hipMemcpyAsync(I->d_wlive + slot, &zero, 4, hipMemcpyHostToDevice, I->stream);
  (void)hipStreamSynchronize(I->stream);
}

bool Slab::EventRingInit(int64_t cap, std::string* err) {
  Impl* I = p;
  if (I->er_keys) return true;
  I->er_cap = cap;
  HIP_CHECK(hipMalloc(&I->er_keys, cap * KEYW));
  HIP_CHECK(hipMalloc(&I->er_rev, cap * 8));
  return true;
}

bool Slab::EventRingPush(const uint8_t* keys96, const uint64_t* revs,
                         int64_t count, int64_t base_seq, std::string* err) {
  Impl* I = p;
  if (!I->er_keys) { if (err) *err = "event ring not initialized"; return false; }
  // contiguous seqs; the ring may wrap once per push
  if (count <= 0) return true;
  if (count > I->er_cap) { if (err) *err = "event push larger than the ring"; return false; }
  int64_t s0 = base_seq % I->er_cap;
  int64_t first = std::min(count, I->er_cap - s0);
  // stage keys|revs in a pinned double-buffered block (the callers' vectors
  // are pageable and die on return) and queue the copies without draining
  // the stream: WatchFilterRing, WatchCatchup and the payload ring queue on
  // the same stream, so they see the pushed span. Slot reuse waits on that
  // slot's own copies only.
  int slot = I->evpush_idx ^= 1;
  if (!I->ev_evpush[slot]) HIP_CHECK(hipEventCreate(&I->ev_evpush[slot]));
  HIP_CHECK(hipEventSynchronize(I->ev_evpush[slot]));
  int64_t need = count * (KEYW + 8);
  if (need > I->h_evpush_cap[slot]) {
    if (I->h_evpush[slot]) (void)hipHostFree(I->h_evpush[slot]);
    I->h_evpush[slot] = nullptr;
    I->h_evpush_cap[slot] = 0;
    int64_t cap = std::max<int64_t>(need, 512 * (KEYW + 8));
    HIP_CHECK(hipHostMalloc(&I->h_evpush[slot], cap));
    I->h_evpush_cap[slot] = cap;
  }
  uint8_t* hk = I->h_evpush[slot];
  uint64_t* hr = (uint64_t*)(hk + count * KEYW);
  memcpy(hk, keys96, count * KEYW);
  memcpy(hr, revs, count * 8);
  HIP_CHECK(hipMemcpyAsync(I->er_keys + s0 * KEYW, hk, first * KEYW,
                           hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipMemcpyAsync(I->er_rev + s0, hr, first * 8,
                           hipMemcpyHostToDevice, I->stream));
  if (first < count) {
    HIP_CHECK(hipMemcpyAsync(I->er_keys, hk + first * KEYW,
                             (count - first) * KEYW, hipMemcpyHostToDevice,
                             I->stream));
    HIP_CHECK(hipMemcpyAsync(I->er_rev, hr + first, (count - first) * 8,
                             hipMemcpyHostToDevice, I->stream));
  }
  HIP_CHECK(hipEventRecord(I->ev_evpush[slot], I->stream));
  return true;
}

bool Slab::WatchFilterRing(int64_t base_seq, int64_t count,
                           std::vector<uint64_t>* bitmap,
                           int64_t* n_watch_slots, std::string* err) {
  Impl* I = p;
  int64_t W = I->wcap;
  *n_watch_slots = W;
  bitmap->clear();
  if (W == 0 || count == 0) return true;
  if (count > 512) { if (err) *err = "filter batch > 512"; return false; }
  int64_t words = ceil_div(count, 64);
  if (W * words > I->bitmap_cap) {
    int64_t cap = W * words * 2;
    if (I->d_bitmap) (void)hipFree(I->d_bitmap);
    HIP_CHECK(hipMalloc(&I->d_bitmap, cap * 8));
    I->bitmap_cap = cap;
  }
  HIP_CHECK(hipEventRecord(I->ev0, I->stream));
  hipLaunchKernelGGL(k_watch_filter2,
                     dim3((uint32_t)ceil_div(W, 64), (uint32_t)words),
                     dim3(64), 0, I->stream, I->er_keys, I->er_rev, I->er_cap,
                     base_seq, count, I->d_wpfx, I->d_wplen, I->d_wfrom,
                     I->d_wlive, W, I->d_bitmap, words);
  HIP_CHECK(hipEventRecord(I->ev1, I->stream));
  bitmap->resize(W * words);
  HIP_CHECK(hipMemcpyAsync(bitmap->data(), I->d_bitmap, W * words * 8,
                           hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev0, I->ev1);
  perf.filter_ms += ms;
  perf.filter_launches++;
  perf.filter_events += count;
  perf.filter_watchers += W;
  return true;
}

bool Slab::WatchCatchup(const uint8_t* pfx96, uint32_t plen, uint64_t from_rev,
                        int64_t base_seq, int64_t count,
                        std::vector<uint64_t>* words_out, std::string* err) {
  Impl* I = p;
  words_out->clear();
  if (count <= 0) return true;
  int64_t words = ceil_div(count, 64);
  if (words > I->bitmap_cap) {
    int64_t cap = words * 2;
    if (I->d_bitmap) (void)hipFree(I->d_bitmap);
    HIP_CHECK(hipMalloc(&I->d_bitmap, cap * 8));
    I->bitmap_cap = cap;
  }
  uint8_t pfx[KEYW] = {0};
  memcpy(pfx, pfx96, plen > (uint32_t)KEYW ? KEYW : plen);
  HIP_CHECK(hipMemcpyAsync(I->d_bkeys, pfx, KEYW, hipMemcpyHostToDevice,
                           I->stream));
  HIP_CHECK(hipEventRecord(I->ev0, I->stream));
  hipLaunchKernelGGL(k_watch_catchup, dim3((uint32_t)ceil_div(count, 256)),
                     dim3(256), 0, I->stream, I->er_keys, I->er_rev, I->er_cap,
                     base_seq, count, I->d_bkeys,
                     plen > (uint32_t)KEYW ? (uint32_t)KEYW : plen, from_rev,
                     I->d_bitmap);
  HIP_CHECK(hipEventRecord(I->ev1, I->stream));
  words_out->resize(words);
  HIP_CHECK(hipMemcpyAsync(words_out->data(), I->d_bitmap, words * 8,
                           hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev0, I->ev1);
  perf.filter_ms += ms;
  perf.filter_launches++;
  perf.filter_events += count;
  perf.filter_watchers += 1;
  return true;
}

// ---- payload ring + batched poll ------------------------------------------

bool Slab::PayloadArm(int64_t ring_bytes, std::string* err) {
  Impl* I = p;
  if (I->pay) return true;
  if (!I->er_keys) { if (err) *err = "event ring not initialized"; return false; }
  if (ring_bytes < 16) { if (err) *err = "payload ring too small"; return false; }
  HIP_CHECK(hipMalloc(&I->er_poff, I->er_cap * 8));
  HIP_CHECK(hipMalloc(&I->er_plen, I->er_cap * 4));
  HIP_CHECK(hipMemsetAsync(I->er_poff, 0, I->er_cap * 8, I->stream));
  HIP_CHECK(hipMemsetAsync(I->er_plen, 0, I->er_cap * 4, I->stream));
  HIP_CHECK(hipEventCreate(&I->ev_w0));
  HIP_CHECK(hipEventCreate(&I->ev_w1));
  HIP_CHECK(hipEventCreate(&I->ev_w2));
  HIP_CHECK(hipMalloc(&I->pay, ring_bytes));
  I->pay_cap = ring_bytes;
  HIP_CHECK(hipStreamSynchronize(I->stream));
  return true;
}

uint8_t* Slab::PayloadStaging(int64_t need, std::string* err) {
  Impl* I = p;
  if (need > I->h_pstage_cap) {
    if (I->h_pstage) (void)hipHostFree(I->h_pstage);
    I->h_pstage = nullptr;
    I->h_pstage_cap = 0;
    int64_t cap = std::max<int64_t>(1 << 20, need + need / 2);
    HIP_CHECK_NULL(hipHostMalloc(&I->h_pstage, cap));
    I->h_pstage_cap = cap;
  }
  return I->h_pstage;
}

bool Slab::PayloadPush(const PaySeg* segs, size_t nsegs, const uint64_t* poffs,
                       const uint32_t* plens, int64_t count, int64_t base_seq,
                       std::string* err) {
  Impl* I = p;
  if (!I->pay) { if (err) *err = "payload ring not armed"; return false; }
  for (size_t i = 0; i < nsegs; ++i) {
    const PaySeg& s = segs[i];
    if (s.len <= 0) continue;
    if (s.ring_off < 0 || s.ring_off + s.len > I->pay_cap || s.stage_off < 0 ||
        s.stage_off + s.len > I->h_pstage_cap) {
      if (err) *err = "payload segment out of bounds";
      return false;
    }
    HIP_CHECK(hipMemcpyAsync(I->pay + s.ring_off, I->h_pstage + s.stage_off,
                             s.len, hipMemcpyHostToDevice, I->stream));
  }
  // column entries; contiguous seqs, the ring may wrap once per push
  int64_t s0 = base_seq % I->er_cap;
  int64_t first = std::min(count, I->er_cap - s0);
  HIP_CHECK(hipMemcpyAsync(I->er_poff + s0, poffs, first * 8,
                           hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipMemcpyAsync(I->er_plen + s0, plens, first * 4,
                           hipMemcpyHostToDevice, I->stream));
  if (first < count) {
    HIP_CHECK(hipMemcpyAsync(I->er_poff, poffs + first, (count - first) * 8,
                             hipMemcpyHostToDevice, I->stream));
    HIP_CHECK(hipMemcpyAsync(I->er_plen, plens + first, (count - first) * 4,
                             hipMemcpyHostToDevice, I->stream));
  }
  // the staging buffer and the caller's vectors are reused by the next push
  HIP_CHECK(hipStreamSynchronize(I->stream));
  return true;
}

WpollRef* Slab::WpollRefStaging(int64_t nrefs, std::string* err) {
  if (!p->ensure_wrefs(nrefs, err)) return nullptr;
  return p->h_wrefs;
}

uint64_t* Slab::WpollOffStaging(int64_t nrefs, std::string* err) {
  if (!p->ensure_wrefs(nrefs, err)) return nullptr;
  return p->h_woffs;
}

bool Slab::WpollSizeRefs(int64_t nrefs, const WpollSize** sizes,
                         std::string* err) {
  Impl* I = p;
  if (!I->pay || nrefs <= 0 || nrefs > I->wrefs_cap) {
    if (err) *err = "wpoll: not armed or bad ref count";
    return false;
  }
  HIP_CHECK(hipMemcpyAsync(I->d_wrefs, I->h_wrefs, nrefs * sizeof(WpollRef),
                           hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_w0, I->stream));
  (void)hipGetLastError();  // drop stale sticky errors: check OUR launch
  hipLaunchKernelGGL(k_wpoll_size, dim3((uint32_t)ceil_div(nrefs, 4)),
                     dim3(256), 0, I->stream, I->d_wrefs, nrefs, I->er_plen,
                     I->er_cap, I->d_wsizes);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(I->ev_w1, I->stream));
  HIP_CHECK(hipMemcpyAsync(I->h_wsizes, I->d_wsizes, nrefs * sizeof(WpollSize),
                           hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_w0, I->ev_w1);
  perf.wpoll_ms += ms;
  perf.wpoll_launches++;
  *sizes = I->h_wsizes;
  return true;
}

bool Slab::WpollEmit(int64_t nrefs, int64_t lo, int64_t hi, int64_t total,
                     uint8_t** reply, std::string* err) {
  Impl* I = p;
  if (!I->pay || nrefs <= 0 || nrefs > I->wrefs_cap || lo < 0 || hi < lo ||
      hi > total) {
    if (err) *err = "wpoll: not armed or bad emit span";
    return false;
  }
  if (total > I->warena_cap) {
    if (I->d_warena) (void)hipFree(I->d_warena);
    I->d_warena = nullptr;
    I->warena_cap = 0;
    int64_t cap = std::max<int64_t>(1 << 20, total + total / 2);
    // +16: the copy's aligned 16 B loads never leave a record's padded
    // extent, the slack keeps the arena's last store inside the allocation
    HIP_CHECK(hipMalloc(&I->d_warena, cap + 16));
    I->warena_cap = cap;
  }
  if (total > I->wreply_cap) {
    if (I->h_wreply) (void)hipHostFree(I->h_wreply);
    I->h_wreply = nullptr;
    I->wreply_cap = 0;
    int64_t cap = std::max<int64_t>(1 << 20, total + total / 2);
    HIP_CHECK(hipHostMalloc(&I->h_wreply, cap));
    I->wreply_cap = cap;
  }
  HIP_CHECK(hipMemcpyAsync(I->d_woffs, I->h_woffs, nrefs * 8,
                           hipMemcpyHostToDevice, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_w0, I->stream));
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_wpoll_emit, dim3((uint32_t)ceil_div(nrefs, 4)),
                     dim3(256), 0, I->stream, I->d_wrefs, I->d_woffs, nrefs,
                     I->er_poff, I->er_plen, I->er_cap, I->pay, I->pay_cap,
                     I->d_warena, total);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(I->ev_w1, I->stream));
  if (hi > lo)
    HIP_CHECK(hipMemcpyAsync(I->h_wreply + lo, I->d_warena + lo, hi - lo,
                             hipMemcpyDeviceToHost, I->stream));
  HIP_CHECK(hipEventRecord(I->ev_w2, I->stream));
  HIP_CHECK(hipStreamSynchronize(I->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_w0, I->ev_w1);
  perf.wpoll_ms += ms;
  ms = 0;
  (void)hipEventElapsedTime(&ms, I->ev_w1, I->ev_w2);
  perf.wpoll_d2h_ms += ms;
  perf.wpoll_launches++;
  perf.wpoll_bytes += hi - lo;
  *reply = I->h_wreply;
  return true;
}

}  // namespace kbslab
