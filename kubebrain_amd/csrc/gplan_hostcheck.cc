// kubebrain_amd/csrc/gplan_hostcheck.cc — stand-alone CPU check of the pure
// host half of the batched point read (gplan.h): the reply planner and its
// emit rounds, on fixed cases and against a brute-force model. No HIP, no
// store; meant to be built with sanitizers:
//   make -C kubebrain_amd/csrc get-hostcheck        (plain)
//   make -C kubebrain_amd/csrc get-hostcheck-asan   (-fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>

#include "gplan.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

using kbget::Plan;
using kbget::PlanOut;

static int check_fixed() {
  // value 100, not found, empty value, value 60
  int32_t hk[4] = {1, 0, 1, 1};
  uint64_t vl[4] = {100, 0, 0, 60};
  PlanOut o;
  CHECK(Plan(hk, vl, 4, 1024, 1 << 20, 1 << 20, &o) == kbget::P_OK);
  CHECK(o.required == 4 + 4 * 32 + 160 && o.found == 3 && o.n_host == 0);
  CHECK(o.val_off[0] == 132 && o.val_off[1] == 232 && o.val_off[2] == 232 &&
        o.val_off[3] == 232);
  CHECK(o.round[0] == 0 && o.round[1] == -1 && o.round[2] == -1 && o.round[3] == 0);
  CHECK(o.round_lo.size() == 1 && o.round_lo[0] == 0 && o.round_hi[0] == 4);
  const uint64_t req = o.required;
  CHECK(Plan(hk, vl, 4, 1024, req - 1, 1 << 20, &o) == kbget::P_ENOBUF);
  CHECK(o.required == req && o.round_lo.size() == 1);
  CHECK(Plan(hk, vl, 4, 1024, 3, 1 << 20, &o) == kbget::P_ENOBUF && o.required == req);
  CHECK(Plan(hk, vl, 4, 1024, req, 1 << 20, &o) == kbget::P_OK);
  // arena of 159: two rounds; of 160: one; of 100: value 0 fits exactly
  CHECK(Plan(hk, vl, 4, 1024, req, 159, &o) == kbget::P_OK);
  CHECK(o.round_lo.size() == 2 && o.round[0] == 0 && o.round[3] == 1);
  CHECK(o.round_lo[0] == 0 && o.round_hi[0] == 1 && o.round_lo[1] == 3 && o.round_hi[1] == 4);
  CHECK(Plan(hk, vl, 4, 1024, req, 160, &o) == kbget::P_OK && o.round_lo.size() == 1);
  CHECK(Plan(hk, vl, 4, 1024, req, 100, &o) == kbget::P_OK);
  CHECK(o.round_lo.size() == 2 && o.n_host == 0);
  // one byte less: value 0 alone exceeds the arena -> host path, no round
  CHECK(Plan(hk, vl, 4, 1024, req, 99, &o) == kbget::P_OK);
  CHECK(o.n_host == 1 && o.round[0] == kbget::R_HOST && o.round[3] == 0 &&
        o.round_lo.size() == 1 && o.round_lo[0] == 3 && o.val_off[3] == 232);
  // sub-batches of 2 never share a round
  uint64_t v2[4] = {10, 10, 10, 10};
  int32_t h2[4] = {1, 1, 1, 1};
  CHECK(Plan(h2, v2, 4, 2, 1 << 20, 1 << 20, &o) == kbget::P_OK);
  CHECK(o.round_lo.size() == 2 && o.round[1] == 0 && o.round[2] == 1);
  // a host-path query between two rounds, first and last
  uint64_t v3[5] = {500, 10, 500, 10, 500};
  int32_t h3[5] = {1, 1, 1, 1, 1};
  CHECK(Plan(h3, v3, 5, 1024, 1 << 20, 64, &o) == kbget::P_OK);
  CHECK(o.n_host == 3 && o.round_lo.size() == 2 && o.round[1] == 0 && o.round[3] == 1);
  // invalid inputs
  uint64_t bad[1] = {7};
  int32_t nk[1] = {0};
  CHECK(Plan(nk, bad, 1, 1024, 100, 100, &o) == kbget::P_EINVALID);
  CHECK(Plan(h2, v2, 4, 0, 100, 100, &o) == kbget::P_EINVALID);
  // zero queries
  CHECK(Plan(nullptr, nullptr, 0, 1024, 4, 64, &o) == kbget::P_OK && o.required == 4);
  CHECK(Plan(nullptr, nullptr, 0, 1024, 3, 64, &o) == kbget::P_ENOBUF && o.required == 4);
  return 0;
}

static uint64_t rnd(uint64_t* s) {
  *s = *s * 6364136223846793005ull + 1442695040888963407ull;
  return *s >> 33;
}

static int check_random() {
  uint64_t seed = 0x6e7;
  for (int it = 0; it < 2000; ++it) {
    const size_t n = rnd(&seed) % 60;
    const size_t max_q = 1 + rnd(&seed) % 20;
    const uint64_t arena = 1 + rnd(&seed) % 3000;
    std::vector<int32_t> hk(n);
    std::vector<uint64_t> vl(n);
    uint64_t sum = 0, found = 0;
    for (size_t i = 0; i < n; ++i) {
      hk[i] = rnd(&seed) % 4 != 0;
      vl[i] = hk[i] && rnd(&seed) % 5 ? rnd(&seed) % 4000 : 0;
      sum += vl[i];
      found += hk[i];
    }
    PlanOut o;
    const uint64_t req = 4 + 32 * (uint64_t)n + sum;
    CHECK(Plan(hk.data(), vl.data(), n, max_q, req, arena, &o) == kbget::P_OK);
    CHECK(o.required == req && o.found == found);
    CHECK(o.round_lo.size() == o.round_hi.size());
    uint64_t off = 4 + 32 * (uint64_t)n, host = 0;
    int32_t last = -1;
    for (size_t i = 0; i < n; ++i) {
      CHECK(o.val_off[i] == off);
      off += vl[i];
      if (vl[i] == 0) { CHECK(o.round[i] == kbget::R_NONE); continue; }
      if (vl[i] > arena) { CHECK(o.round[i] == kbget::R_HOST); ++host; continue; }
      CHECK(o.round[i] == last || o.round[i] == last + 1);
      last = o.round[i];
    }
    CHECK(host == o.n_host && (size_t)(last + 1) == o.round_lo.size());
    for (size_t r = 0; r < o.round_lo.size(); ++r) {
      const size_t lo = (size_t)o.round_lo[r], hi = (size_t)o.round_hi[r];
      CHECK(lo < hi && hi <= n && lo / max_q == (hi - 1) / max_q);
      CHECK(o.round[lo] == (int32_t)r && o.round[hi - 1] == (int32_t)r);
      uint64_t fill = 0;
      for (size_t i = lo; i < hi; ++i) {
        CHECK(o.round[i] == (int32_t)r || o.round[i] == kbget::R_NONE);
        fill += vl[i];
      }
      CHECK(fill <= arena && fill > 0);
      // maximal: the next value-carrying query did not fit, or is host
      // path, or lies in the next sub-batch
      size_t nx = hi;
      while (nx < n && vl[nx] == 0) ++nx;
      if (nx < n && nx / max_q == lo / max_q && vl[nx] <= arena)
        CHECK(fill + vl[nx] > arena);
    }
    if (req > 0)
      CHECK(Plan(hk.data(), vl.data(), n, max_q, req - 1, arena, &o) == kbget::P_ENOBUF);
    CHECK(o.required == req);
  }
  return 0;
}

int main() {
  if (check_fixed()) return 1;
  if (check_random()) return 1;
  printf("gplan_hostcheck OK\n");
  return 0;
}
