// kubebrain_amd/csrc/dmerge.h — slot arithmetic of the small-insert merge
// (slab.hip k_delta_scatter): m sorted new rows go into a sorted run of n old
// rows; a new row whose (key, rev) equals an old row's replaces that row.
// Host and device share these functions, so dmerge_hostcheck.cc proves them
// against a naive merge on the CPU.
//
// Inputs, for new row j in [0, m):
//   lb[j]   = first old row with (key, rev) >= new row j; non-decreasing in j
//   dup[j]  = old row lb[j] equals new row j (that old row is dropped). New
//             rows are strictly increasing, so at most one new row is the dup
//             of an old row, and it is the last of the new rows sharing its lb
//   dupx[j] = dup[0] + ... + dup[j-1], for j in [0, m]
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define KBM_HD __host__ __device__
#else
#define KBM_HD
#endif

namespace kbmerge {

constexpr int kMaxNew = 1024;  // new rows of one small insert (fits LDS)

// number of entries of the non-decreasing lb[0, m) below x
KBM_HD inline int CountLess(const int64_t* lb, int m, int64_t x) {
  int lo = 0, hi = m;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (lb[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ... at or below x
KBM_HD inline int CountLessEq(const int64_t* lb, int m, int64_t x) {
  int lo = 0, hi = m;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (lb[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// slot of old row i in the merged run, -1 if a new row replaces it. With
// p = #{j : lb[j] < i} and q = #{j : lb[j] <= i}, new rows [p, q) share the
// insertion point i and only the last of them can be its dup. A surviving
// row moves up by the q new rows in front of it and down by the dupx[p]
// old rows dropped before it.
KBM_HD inline int64_t OldSlot(int64_t i, const int64_t* lb,
                              const uint16_t* dupx, int m) {
  const int p = CountLess(lb, m, i), q = CountLessEq(lb, m, i);
  if (q > p && dupx[q] != dupx[q - 1]) return -1;
  return i + q - (int64_t)dupx[p];
}

// slot of new row j: behind the lb[j] old rows in front of it less the
// dupx[j] of them that were dropped, and behind the j new rows before it
KBM_HD inline int64_t NewSlot(int j, const int64_t* lb, const uint16_t* dupx) {
  return lb[j] + j - (int64_t)dupx[j];
}

// rows of the merged run
KBM_HD inline int64_t NewCount(int64_t n, int m, const uint16_t* dupx) {
  return n + m - (int64_t)dupx[m];
}

}  // namespace kbmerge
