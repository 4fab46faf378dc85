// kubebrain_amd/csrc/stepstage.h — pure host layout arithmetic of the bench
// step's upload blocks: the step staging block that carries
// a step's get queries, range queries and key tails in ONE host-to-device
// copy, and the delta-row block that carries keys|meta|rev|vo|ko of m new
// rows in one more. No HIP calls and no store state, so a stand-alone
// sanitizer build (stepstage_hostcheck.cc) can exercise it without a GPU.
#pragma once

#include <cstdint>

namespace kbstage {

constexpr int64_t kAlign = 16;
constexpr int64_t align_up(int64_t x) { return (x + kAlign - 1) & ~(kAlign - 1); }

// One step's slices, as byte offsets from the start of the block. The same
// offsets hold in the pinned mirror and in the device allocation, so the
// upload is the single span [0, total).
struct StepLayout {
  int64_t off_getq = 0;   // nget  x getq_bytes
  int64_t off_rangeq = 0; // nrange x rangeq_bytes
  int64_t off_tails = 0;  // tail_cap bytes at most; the step uses tail_bytes
  int64_t tail_cap = 0;   // room left for tails behind the queries
};

// Capacity of a block that holds max_q queries of either kind plus
// tail_bytes of key tails.
inline int64_t StepCapacity(int64_t max_q, int64_t getq_bytes,
                            int64_t rangeq_bytes, int64_t tail_bytes) {
  return align_up(max_q * getq_bytes) + align_up(max_q * rangeq_bytes) +
         align_up(tail_bytes);
}

// Lays nget get queries, nrange range queries and the tails out in a block
// of `capacity` bytes. False when a count is negative or above max_q, or the
// queries alone do not fit. Slices are 16 B aligned and never overlap.
inline bool PlanStep(int64_t nget, int64_t nrange, int64_t max_q,
                     int64_t getq_bytes, int64_t rangeq_bytes,
                     int64_t capacity, StepLayout* o) {
  if (nget < 0 || nrange < 0 || nget > max_q || nrange > max_q) return false;
  if (getq_bytes <= 0 || rangeq_bytes <= 0 || capacity < 0) return false;
  o->off_getq = 0;
  o->off_rangeq = align_up(nget * getq_bytes);
  o->off_tails = o->off_rangeq + align_up(nrange * rangeq_bytes);
  if (o->off_tails > capacity) return false;
  o->tail_cap = capacity - o->off_tails;
  return true;
}

// Bytes of the one upload for a step that used tail_bytes of its tail slice;
// -1 when the tails overflow it.
inline int64_t StepSpan(const StepLayout& l, int64_t tail_bytes) {
  if (tail_bytes < 0 || tail_bytes > l.tail_cap) return -1;
  return l.off_tails + tail_bytes;
}

// Delta rows: five columns with stride m (not the block's row capacity), so
// the m rows of a call are one contiguous span.
struct RowLayout {
  int64_t off_keys = 0, off_meta = 0, off_rev = 0, off_vo = 0, off_ko = 0;
  int64_t total = 0;
};

inline bool PlanRows(int64_t m, int64_t row_cap, int64_t keyw, RowLayout* o) {
  if (m <= 0 || m > row_cap || keyw <= 0 || keyw % 8 != 0) return false;
  o->off_keys = 0;
  o->off_meta = m * keyw;
  o->off_rev = o->off_meta + m * 8;
  o->off_vo = o->off_rev + m * 8;
  o->off_ko = o->off_vo + m * 8;
  o->total = o->off_ko + m * 8;
  return true;
}

}  // namespace kbstage
