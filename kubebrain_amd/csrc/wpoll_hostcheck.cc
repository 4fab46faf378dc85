// kubebrain_amd/csrc/wpoll_hostcheck.cc — stand-alone CPU check of the pure
// host half of the batched watch poll (wpoll.h): payload-ring placement
// against a brute-force byte-ownership model, the reply planner and the
// record serializer. No HIP, no store; meant to be built with sanitizers:
//   make -C kubebrain_amd/csrc hostcheck        (plain)
//   make -C kubebrain_amd/csrc hostcheck-asan   (-fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

#include "wpoll.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static int check_ring() {
  srand(7);
  for (int trial = 0; trial < 200; ++trial) {
    kbwpoll::PayRing r;
    int64_t cap = 64 + 16 * (rand() % 200), slots = 8 + rand() % 100;
    int64_t seq0 = rand() % 50;
    r.init(cap, slots, seq0);
    std::vector<int64_t> owner((size_t)cap, -1);  // byte -> owning seq
    std::map<int64_t, std::pair<int64_t, int64_t>> placed;
    for (int64_t seq = seq0; seq < seq0 + 600; ++seq) {
      uint64_t len = 28 + rand() % (rand() % 8 == 0 ? 4000 : 300);
      int64_t at = r.place(seq, len);
      int64_t al = (int64_t)((len + 15) & ~15ull);
      if (at < 0) {  // larger than the ring: window emptied through seq
        CHECK(al > cap);
        CHECK(r.oldest_seq == seq + 1);
        continue;
      }
      CHECK(at % 16 == 0 && at + al <= cap);  // aligned, never straddles
      for (int64_t b = at; b < at + al; ++b) owner[(size_t)b] = seq;
      placed[seq] = {at, al};
      // every event of the resident window is placed and fully intact
      CHECK(r.oldest_seq <= seq && r.oldest_seq >= seq + 1 - slots);
      for (int64_t q = r.oldest_seq; q <= seq; ++q) {
        auto it = placed.find(q);
        CHECK(it != placed.end());
        for (int64_t b = it->second.first;
             b < it->second.first + it->second.second; ++b)
          CHECK(owner[(size_t)b] == q);
        CHECK((int64_t)r.poff[(size_t)(q % slots)] == it->second.first);
      }
    }
  }
  return 0;
}

static int check_plan() {
  kbwpoll::PlanRef refs[3] = {{100, 2, 0}, {50, 1, 0}, {7, 1, 3}};
  int32_t st[4] = {0, 10, 0, 0};
  int64_t hl[4] = {-1, 0, 44, -1};
  kbwpoll::PlanOut o;
  CHECK(kbwpoll::Plan(refs, 3, st, hl, 4, 1 << 20, &o) == kbwpoll::P_OK);
  CHECK(o.required == 4 + 8 + 154 + 8 + 0 + 8 + 44 + 8 + 11);
  CHECK(o.ref_off[0] == 16 && o.ref_off[1] == 116);
  CHECK(o.dev_lo == 16 && o.dev_hi == o.required);
  uint64_t req = o.required;
  CHECK(kbwpoll::Plan(refs, 3, st, hl, 4, req - 1, &o) == kbwpoll::P_ENOBUF);
  CHECK(o.required == req);
  std::vector<uint8_t> out((size_t)req);
  kbwpoll::WriteDirectory(out.data(), st, 4, o);
  kbwpoll::PlanRef bad[1] = {{1, 1, 1}};
  CHECK(kbwpoll::Plan(bad, 1, st, hl, 4, 1 << 20, &o) == kbwpoll::P_EINVALID);
  CHECK(kbwpoll::Plan(nullptr, 0, nullptr, nullptr, 0, 3, &o) ==
        kbwpoll::P_ENOBUF);
  CHECK(o.required == 4);
  return 0;
}

static int check_record() {
  uint8_t buf[64];
  uint8_t* e = kbwpoll::PutRecord(buf, 2, 5, 4, "ab", 2, "xyz", 3);
  CHECK((size_t)(e - buf) == kbwpoll::RecordSize(2, 3));
  CHECK(buf[0] == 2 && buf[4] == 5 && buf[12] == 4 && buf[20] == 2);
  CHECK(buf[24] == 'a' && buf[26] == 3 && buf[30] == 'x');
  e = kbwpoll::PutRecord(buf, 0, 5, 5, nullptr, 0, nullptr, 0);
  CHECK(e - buf == 28);
  return 0;
}

int main() {
  if (check_ring() || check_plan() || check_record()) return 1;
  printf("wpoll host checks OK\n");
  return 0;
}
