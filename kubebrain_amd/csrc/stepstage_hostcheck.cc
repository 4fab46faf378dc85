// kubebrain_amd/csrc/stepstage_hostcheck.cc — stand-alone CPU check of the
// bench step's upload layouts (stepstage.h): every slice is written into a
// heap block of exactly the planned capacity and read back, so an overlap or
// an overrun shows as a wrong byte or as a sanitizer report. No HIP, no
// store; meant to be built with sanitizers:
//   make -C kubebrain_amd/csrc step-hostcheck        (plain)
//   make -C kubebrain_amd/csrc step-hostcheck-asan   (-fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stepstage.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

using namespace kbstage;

// sizes of the packed device query structs (slab_dev.h DevGetQ / DevRangeQ)
constexpr int64_t kGetQ = 120, kRangeQ = 248;
constexpr int64_t kMaxQ = 1024;

// fill [off, off+len) with tag; every byte must have been untouched (0)
static int fill(std::vector<uint8_t>* blk, int64_t off, int64_t len, uint8_t tag) {
  CHECK(off >= 0 && len >= 0 && off + len <= (int64_t)blk->size());
  for (int64_t i = 0; i < len; ++i) {
    CHECK((*blk)[off + i] == 0);
    (*blk)[off + i] = tag;
  }
  return 0;
}

static int check_step() {
  const int64_t tail_room = 8192;
  const int64_t cap = StepCapacity(kMaxQ, kGetQ, kRangeQ, tail_room);
  CHECK(cap % kAlign == 0);
  CHECK(cap >= kMaxQ * (kGetQ + kRangeQ) + tail_room);
  const int64_t nqs[] = {0, 1, kMaxQ};
  const int64_t ntxs[] = {0, 1, 1024};
  const int64_t tails[] = {0, 1, 4097};
  for (int64_t nq : nqs)
    for (int64_t ntx : ntxs)
      for (int64_t tb : tails) {
        StepLayout l;
        CHECK(PlanStep(ntx, nq, kMaxQ, kGetQ, kRangeQ, cap, &l));
        CHECK(l.off_getq % kAlign == 0 && l.off_rangeq % kAlign == 0 &&
              l.off_tails % kAlign == 0);
        CHECK(l.off_getq == 0);
        CHECK(l.off_rangeq >= l.off_getq + ntx * kGetQ);
        CHECK(l.off_tails >= l.off_rangeq + nq * kRangeQ);
        CHECK(l.tail_cap >= tail_room);  // even at max_q of both kinds
        CHECK(l.off_tails + l.tail_cap == cap);
        const int64_t span = StepSpan(l, tb);
        CHECK(span == l.off_tails + tb && span <= cap);
        std::vector<uint8_t> blk((size_t)cap, 0);
        if (fill(&blk, l.off_getq, ntx * kGetQ, 1)) return 1;
        if (fill(&blk, l.off_rangeq, nq * kRangeQ, 2)) return 1;
        if (fill(&blk, l.off_tails, tb, 3)) return 1;
        // the one upload [0, span) carries every written byte
        for (int64_t i = span; i < cap; ++i) CHECK(blk[(size_t)i] == 0);
        // one byte more than the tail slice holds is rejected
        CHECK(StepSpan(l, l.tail_cap) == cap);
        CHECK(StepSpan(l, l.tail_cap + 1) == -1);
        CHECK(StepSpan(l, -1) == -1);
      }
  StepLayout l;
  // counts above max_q, negative counts, a block too small for the queries
  CHECK(!PlanStep(kMaxQ + 1, 0, kMaxQ, kGetQ, kRangeQ, cap, &l));
  CHECK(!PlanStep(0, kMaxQ + 1, kMaxQ, kGetQ, kRangeQ, cap, &l));
  CHECK(!PlanStep(-1, 0, kMaxQ, kGetQ, kRangeQ, cap, &l));
  CHECK(!PlanStep(0, -1, kMaxQ, kGetQ, kRangeQ, cap, &l));
  CHECK(!PlanStep(1, 1, kMaxQ, kGetQ, kRangeQ, kGetQ + kRangeQ, &l));  // needs 128 + 256
  CHECK(PlanStep(1, 1, kMaxQ, kGetQ, kRangeQ, 128 + 256, &l) && l.tail_cap == 0);
  CHECK(StepSpan(l, 0) == 384 && StepSpan(l, 1) == -1);
  CHECK(!PlanStep(1, 1, kMaxQ, 0, kRangeQ, cap, &l));
  // a get query size that is no multiple of 16 still aligns the next slice
  CHECK(PlanStep(3, 2, kMaxQ, 121, 233, cap, &l));
  CHECK(l.off_rangeq == 368 && l.off_tails == 368 + 480);
  return 0;
}

static int check_rows() {
  const int64_t keyw = 96;
  const int64_t ms[] = {1, 3, 1024};
  for (int64_t m : ms) {
    const int64_t row_cap = m + m / 2 + 1024;  // Impl::ensure_delta's growth
    RowLayout l;
    CHECK(PlanRows(m, row_cap, keyw, &l));
    CHECK(l.off_keys == 0 && l.off_meta == m * keyw);
    CHECK(l.off_rev == l.off_meta + m * 8 && l.off_vo == l.off_rev + m * 8 &&
          l.off_ko == l.off_vo + m * 8);
    CHECK(l.total == m * (keyw + 32));
    CHECK(l.total <= row_cap * (keyw + 32));
    // u64 columns stay 8 B aligned, the key column 16 B
    CHECK(l.off_meta % 8 == 0 && l.off_rev % 8 == 0 && l.off_vo % 8 == 0 &&
          l.off_ko % 8 == 0 && l.off_keys % 16 == 0);
    std::vector<uint8_t> blk((size_t)l.total, 0);
    if (fill(&blk, l.off_keys, m * keyw, 1)) return 1;
    if (fill(&blk, l.off_meta, m * 8, 2)) return 1;
    if (fill(&blk, l.off_rev, m * 8, 3)) return 1;
    if (fill(&blk, l.off_vo, m * 8, 4)) return 1;
    if (fill(&blk, l.off_ko, m * 8, 5)) return 1;
    for (uint8_t b : blk) CHECK(b != 0);  // contiguous: no hole in the span
  }
  RowLayout l;
  CHECK(!PlanRows(0, 1024, keyw, &l));
  CHECK(!PlanRows(-1, 1024, keyw, &l));
  CHECK(!PlanRows(1025, 1024, keyw, &l));
  CHECK(PlanRows(1024, 1024, keyw, &l));
  CHECK(!PlanRows(1, 1024, 97, &l));
  return 0;
}

int main() {
  if (check_step()) return 1;
  if (check_rows()) return 1;
  printf("stepstage hostcheck OK\n");
  return 0;
}
