// kubebrain_amd/csrc/dmerge_hostcheck.cc — stand-alone CPU check of the
// small-insert merge's slot arithmetic (dmerge.h) against a naive merge:
// exhaustively for every n <= 6, m <= 4 and every valid monotone lb/dup
// assignment, then seeded random cases up to n = 300, m = 64. The slots must
// be a permutation onto [0, new_n) that keeps the order inside the old rows
// and inside the new rows and equals the naive merge's order. No HIP, no
// store; meant to be built with sanitizers:
//   make -C kubebrain_amd/csrc dmerge-hostcheck        (plain)
//   make -C kubebrain_amd/csrc dmerge-hostcheck-asan   (-fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dmerge.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

using namespace kbmerge;

// valid: lb non-decreasing in [0, n]; dup[j] needs lb[j] < n and must be the
// last new row at its lb (new row j+1 sorts after old row lb[j])
static bool valid(int64_t n, const std::vector<int64_t>& lb,
                  const std::vector<int>& dup) {
  const int m = (int)lb.size();
  for (int j = 0; j < m; ++j) {
    if (lb[j] < 0 || lb[j] > n) return false;
    if (j && lb[j] < lb[j - 1]) return false;
    if (dup[j] && lb[j] >= n) return false;
    if (dup[j] && j + 1 < m && lb[j + 1] <= lb[j]) return false;
  }
  return true;
}

// the merged run as a list of tags: old row i -> i, new row j -> -(j + 1).
// Walks the old rows and puts new row j in front of old row lb[j]; a dup
// takes that old row's place.
static std::vector<int64_t> naive(int64_t n, const std::vector<int64_t>& lb,
                                  const std::vector<int>& dup) {
  const int m = (int)lb.size();
  std::vector<int64_t> out;
  int j = 0;
  for (int64_t i = 0; i <= n; ++i) {
    bool dropped = false;
    while (j < m && lb[j] == i) {
      out.push_back(-(int64_t)(j + 1));
      dropped = dropped || dup[j];
      ++j;
    }
    if (i < n && !dropped) out.push_back(i);
  }
  return out;
}

static int check_case(int64_t n, const std::vector<int64_t>& lb,
                      const std::vector<int>& dup) {
  const int m = (int)lb.size();
  // arrays of exactly the used size, so that an overrun is a sanitizer report
  std::vector<uint16_t> dupx((size_t)m + 1);
  dupx[0] = 0;
  for (int j = 0; j < m; ++j) dupx[j + 1] = (uint16_t)(dupx[j] + (dup[j] ? 1 : 0));
  const std::vector<int64_t> want = naive(n, lb, dup);
  const int64_t new_n = NewCount(n, m, dupx.data());
  CHECK(new_n == (int64_t)want.size());
  const int64_t kFree = INT64_MIN;
  std::vector<int64_t> got((size_t)new_n, kFree);
  int64_t prev = -1;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t s = OldSlot(i, lb.data(), dupx.data(), m);
    if (s < 0) continue;
    CHECK(s < new_n && got[(size_t)s] == kFree);
    CHECK(s > prev);  // old rows keep their order
    prev = s;
    got[(size_t)s] = i;
  }
  prev = -1;
  for (int j = 0; j < m; ++j) {
    const int64_t s = NewSlot(j, lb.data(), dupx.data());
    CHECK(s >= 0 && s < new_n && got[(size_t)s] == kFree);
    CHECK(s > prev);  // new rows keep their order
    prev = s;
    got[(size_t)s] = -(int64_t)(j + 1);
  }
  for (int64_t s = 0; s < new_n; ++s) CHECK(got[(size_t)s] == want[(size_t)s]);
  return 0;
}

static int64_t g_cases = 0;

// every lb/dup assignment of m new rows over n old rows
static int enumerate(int64_t n, int m, std::vector<int64_t>* lb,
                     std::vector<int>* dup) {
  if ((int)lb->size() == m) {
    if (!valid(n, *lb, *dup)) return 0;
    ++g_cases;
    return check_case(n, *lb, *dup);
  }
  const int64_t from = lb->empty() ? 0 : lb->back();
  for (int64_t v = from; v <= n; ++v)
    for (int d = 0; d < 2; ++d) {
      lb->push_back(v);
      dup->push_back(d);
      const int rc = enumerate(n, m, lb, dup);
      lb->pop_back();
      dup->pop_back();
      if (rc) return rc;
    }
  return 0;
}

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  g_seed ^= g_seed >> 12;
  g_seed ^= g_seed << 25;
  g_seed ^= g_seed >> 27;
  return g_seed * 0x2545F4914F6CDD1Dull;
}

static int check_random() {
  for (int it = 0; it < 600; ++it) {
    const int64_t n = 1 + (int64_t)(rnd() % 300);
    const int m = 1 + (int)(rnd() % 64);
    // regimes: spread, clustered on few insertion points, all in front, all
    // behind, dup-heavy
    const int regime = it % 5;
    std::vector<int64_t> lb((size_t)m);
    for (int j = 0; j < m; ++j) {
      int64_t v;
      if (regime == 1) v = (int64_t)(rnd() % 3) * (n / 3);
      else if (regime == 2) v = 0;
      else if (regime == 3) v = n;
      else v = (int64_t)(rnd() % (uint64_t)(n + 1));
      lb[(size_t)j] = v;
    }
    // sort (insertion sort: m <= 64)
    for (int a = 1; a < m; ++a)
      for (int b = a; b > 0 && lb[(size_t)b] < lb[(size_t)b - 1]; --b) {
        int64_t t = lb[(size_t)b];
        lb[(size_t)b] = lb[(size_t)b - 1];
        lb[(size_t)b - 1] = t;
      }
    std::vector<int> dup((size_t)m, 0);
    for (int j = 0; j < m; ++j) {
      const bool last = j + 1 == m || lb[(size_t)j + 1] > lb[(size_t)j];
      const bool want = regime == 4 ? true : (rnd() & 1);
      dup[(size_t)j] = last && lb[(size_t)j] < n && want;
    }
    CHECK(valid(n, lb, dup));
    ++g_cases;
    if (check_case(n, lb, dup)) {
      fprintf(stderr, "random case %d (n=%lld m=%d regime=%d) failed\n", it,
              (long long)n, m, regime);
      return 1;
    }
  }
  return 0;
}

int main() {
  for (int64_t n = 0; n <= 6; ++n)
    for (int m = 0; m <= 4; ++m) {
      std::vector<int64_t> lb;
      std::vector<int> dup;
      if (enumerate(n, m, &lb, &dup)) {
        fprintf(stderr, "exhaustive n=%lld m=%d failed\n", (long long)n, m);
        return 1;
      }
    }
  const int64_t exhaustive = g_cases;
  CHECK(exhaustive > 1000);
  if (check_random()) return 1;
  printf("dmerge hostcheck OK (%lld exhaustive + %lld random cases)\n",
         (long long)exhaustive, (long long)(g_cases - exhaustive));
  return 0;
}
