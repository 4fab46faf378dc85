// kubebrain_amd/csrc/lplan_hostcheck.cc — stand-alone CPU check of the pure
// host half of the batched List (lplan.h): the reply planner and its emit
// rounds against a brute-force model, the directory writer and the record
// serializer. No HIP, no store; meant to be built with sanitizers:
//   make -C kubebrain_amd/csrc list-hostcheck        (plain)
//   make -C kubebrain_amd/csrc list-hostcheck-asan   (-fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>

#include "lplan.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static int check_plan_fixed() {
  // device 100 B, error, host 44 B, device empty
  int32_t st[4] = {0, 5, 0, 0};
  int64_t hl[4] = {-1, 0, 44, -1};
  uint64_t db[4] = {100, 0, 0, 0};
  kblist::PlanOut o;
  CHECK(kblist::Plan(st, hl, db, nullptr, 4, 1 << 20, 1 << 20, &o) == kblist::P_OK);
  CHECK(o.required == 4 + 4 * 24 + 104 + 0 + 44 + 4);
  CHECK(o.sec_off[0] == 100 && o.sec_off[1] == 204 && o.sec_off[2] == 204 &&
        o.sec_off[3] == 248);
  CHECK(o.len[0] == 104 && o.len[1] == 0 && o.len[2] == 44 && o.len[3] == 4);
  CHECK(o.round[0] == 0 && o.round[1] == -1 && o.round[2] == -1 && o.round[3] == 0);
  CHECK(o.round_lo.size() == 1 && o.round_lo[0] == 100 && o.round_hi[0] == 252);
  const uint64_t req = o.required;
  CHECK(kblist::Plan(st, hl, db, nullptr, 4, req - 1, 1 << 20, &o) == kblist::P_ENOBUF);
  CHECK(o.required == req);
  CHECK(kblist::Plan(st, hl, db, nullptr, 4, req, 1 << 20, &o) == kblist::P_OK);
  // the host section between the two device sections no longer fits the
  // arena span: two rounds
  CHECK(kblist::Plan(st, hl, db, nullptr, 4, req, 120, &o) == kblist::P_OK);
  CHECK(o.round[0] == 0 && o.round[3] == 1 && o.round_lo.size() == 2);
  CHECK(o.round_lo[1] == 248 && o.round_hi[1] == 252 && o.round_hi[0] == 204);
  // a device section larger than the arena is the caller's to reroute
  CHECK(kblist::Plan(st, hl, db, nullptr, 4, req, 103, &o) == kblist::P_EINVALID);
  // two groups never share a round
  int32_t gr[4] = {0, -1, -1, 1};
  CHECK(kblist::Plan(st, hl, db, gr, 4, req, 1 << 20, &o) == kblist::P_OK);
  CHECK(o.round[0] == 0 && o.round[3] == 1);
  // an OK host section is at least its u32 count
  int64_t hl_bad[4] = {-1, 0, 3, -1};
  CHECK(kblist::Plan(st, hl_bad, db, nullptr, 4, req, 1 << 20, &o) == kblist::P_EINVALID);
  // directory bytes
  std::vector<uint8_t> out((size_t)req, 0xAB);
  int32_t more[4] = {1, 0, 0, 0};
  CHECK(kblist::Plan(st, hl, db, nullptr, 4, req, 1 << 20, &o) == kblist::P_OK);
  kblist::WriteDirectory(out.data(), st, more, 77, 4, o);
  CHECK(out[0] == 4 && out[4] == 0 && out[8] == 1 && out[12] == 77 && out[20] == 104);
  CHECK(out[4 + 24] == 5 && out[4 + 24 + 16] == 0 && out[4 + 48 + 16] == 44);
  CHECK(out[100] == 0xAB);  // sections are not the directory writer's
  // zero queries, all-error batches, cap < 4
  CHECK(kblist::Plan(nullptr, nullptr, nullptr, nullptr, 0, 3, 64, &o) == kblist::P_ENOBUF);
  CHECK(o.required == 4);
  CHECK(kblist::Plan(nullptr, nullptr, nullptr, nullptr, 0, 4, 64, &o) == kblist::P_OK);
  int32_t ste[3] = {5, 12, 4};
  int64_t hle[3] = {0, -1, 99};
  uint64_t dbe[3] = {9, 9, 9};
  CHECK(kblist::Plan(ste, hle, dbe, nullptr, 3, 1 << 20, 64, &o) == kblist::P_OK);
  CHECK(o.required == 4 + 72 && o.round_lo.empty());
  CHECK(o.len[0] == 0 && o.len[1] == 0 && o.len[2] == 0);
  return 0;
}

static int check_plan_random() {
  srand(11);
  for (int trial = 0; trial < 2000; ++trial) {
    const size_t n = (size_t)(rand() % 40);
    const uint64_t arena = 64 + (uint64_t)(rand() % 600);
    std::vector<int32_t> st(n), gr(n);
    std::vector<int64_t> hl(n);
    std::vector<uint64_t> db(n);
    int32_t g = 0;
    for (size_t i = 0; i < n; ++i) {
      st[i] = rand() % 5 == 0 ? 5 : 0;
      const bool host = rand() % 4 == 0;
      hl[i] = host ? 4 + rand() % 900 : -1;
      db[i] = (uint64_t)(rand() % 3 == 0 ? 0 : rand() % (int)(arena - 3));
      if (rand() % 9 == 0) ++g;
      gr[i] = g;
    }
    kblist::PlanOut o;
    CHECK(kblist::Plan(st.data(), hl.data(), db.data(), gr.data(), n, ~0ull,
                       arena, &o) == kblist::P_OK);
    uint64_t off = 4 + 24 * (uint64_t)n;
    int32_t last_round = -1;
    for (size_t i = 0; i < n; ++i) {
      const bool dev = st[i] == 0 && hl[i] < 0;
      const uint64_t len = st[i] != 0 ? 0 : (dev ? 4 + db[i] : (uint64_t)hl[i]);
      CHECK(o.len[i] == len && o.sec_off[i] == off);
      if (dev) {
        const int32_t r = o.round[i];
        CHECK(r == last_round || r == last_round + 1);
        last_round = r;
        CHECK(off >= o.round_lo[(size_t)r] && off + len <= o.round_hi[(size_t)r]);
        CHECK(o.round_hi[(size_t)r] - o.round_lo[(size_t)r] <= arena);
      } else {
        CHECK(o.round[i] == -1);
      }
      off += len;
    }
    CHECK(o.required == off);
    CHECK((size_t)(last_round + 1) == o.round_lo.size());
    // rounds are disjoint, ascending, one group each, and greedy: the next
    // round's first section would not have fitted the previous span
    for (size_t r = 0; r + 1 < o.round_lo.size(); ++r)
      CHECK(o.round_hi[r] <= o.round_lo[r + 1]);
    for (size_t i = 0, prev = n; i < n; ++i) {
      if (o.round[i] < 0) continue;
      if (prev != n && o.round[prev] != o.round[i])
        CHECK(gr[prev] != gr[i] ||
              o.sec_off[i] + o.len[i] - o.round_lo[(size_t)o.round[prev]] > arena);
      if (prev != n && o.round[prev] == o.round[i]) CHECK(gr[prev] == gr[i]);
      prev = i;
    }
    if (off > 0)
      CHECK(kblist::Plan(st.data(), hl.data(), db.data(), gr.data(), n, off - 1,
                         arena, &o) == kblist::P_ENOBUF);
    CHECK(o.required == off);
  }
  return 0;
}

static int check_record() {
  uint8_t buf[64];
  uint8_t* e = kblist::PutRecord(buf, 5, "ab", 2, "xyz", 3);
  CHECK((uint64_t)(e - buf) == kblist::RecordSize(2, 3));
  CHECK(buf[0] == 5 && buf[8] == 2 && buf[12] == 'a' && buf[14] == 3 && buf[18] == 'x');
  e = kblist::PutRecord(buf, 5, nullptr, 0, nullptr, 0);
  CHECK(e - buf == 16);
  return 0;
}

int main() {
  if (check_plan_fixed() || check_plan_random() || check_record()) return 1;
  printf("list plan host checks OK\n");
  return 0;
}
