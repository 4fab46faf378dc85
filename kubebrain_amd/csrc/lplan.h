// kubebrain_amd/csrc/lplan.h — pure host half of the batched Range call
// (kb_list_batch): the kb_list wire-record serializer used by
// the host fallback, the reply planner and the emit-round splitter. No HIP
// calls and no store state, so CPU tests (kb_test_list_plan) and a
// stand-alone sanitizer build can exercise it without a GPU.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace kblist {

// status codes used by the planner (== include/kb_slab.h kb_status)
constexpr int P_OK = 0, P_EINVALID = 5, P_ENOBUF = 100;

// reply = u32 n; n x DirEntry; then the n sections in query order
constexpr uint64_t kDirEntry = 24;  // i32 status; i32 more; u64 header_rev; u64 len

// one kv in kb_list wire form: u64 rev | u32 klen | key | u32 vlen | val
inline uint64_t RecordSize(uint64_t klen, uint64_t vlen) { return 16 + klen + vlen; }

inline uint8_t* PutRecord(uint8_t* p, uint64_t rev, const void* key,
                          uint32_t klen, const void* val, uint32_t vlen) {
  memcpy(p, &rev, 8); p += 8;
  memcpy(p, &klen, 4); p += 4;
  if (klen) memcpy(p, key, klen);
  p += klen;
  memcpy(p, &vlen, 4); p += 4;
  if (vlen) memcpy(p, val, vlen);
  return p + vlen;
}

// Per query i: status[i]; for status OK either host_len[i] >= 4 (a section the
// host serialized, that many bytes) or host_len[i] < 0 (device path: section =
// u32 count + dev_bytes[i] record bytes). Any other status has len 0.
struct PlanOut {
  std::vector<uint64_t> len;      // directory len per query
  std::vector<uint64_t> sec_off;  // reply offset of each query's section
  std::vector<int32_t> round;     // emit round of a device query, else -1
  // per emit round: reply byte span [lo, hi) holding its sections (the arena
  // is laid out like that span, so one D2H moves a whole round)
  std::vector<uint64_t> round_lo, round_hi;
  uint64_t required = 4;
};

// arena_bytes bounds one emit round's span; a device section larger than the
// arena is the caller's to route to the host path beforehand (P_EINVALID).
// Rounds hold whole queries, in query order. group (may be null) names the
// scan sub-batch a device query was sized in: a round never spans two groups,
// because only one sub-batch's winner table is resident at a time.
inline int Plan(const int32_t* status, const int64_t* host_len,
                const uint64_t* dev_bytes, const int32_t* group, size_t n,
                uint64_t cap, uint64_t arena_bytes, PlanOut* o) {
  o->len.assign(n, 0);
  o->sec_off.assign(n, 0);
  o->round.assign(n, -1);
  o->round_lo.clear();
  o->round_hi.clear();
  uint64_t off = 4 + kDirEntry * (uint64_t)n;
  int32_t cur_group = 0;
  for (size_t i = 0; i < n; ++i) {
    uint64_t len = 0;
    const bool dev = status[i] == P_OK && host_len[i] < 0;
    if (status[i] == P_OK && !dev) {
      if (host_len[i] < 4) return P_EINVALID;
      len = (uint64_t)host_len[i];
    } else if (dev) {
      len = 4 + dev_bytes[i];
      if (len > arena_bytes) return P_EINVALID;
    }
    o->len[i] = len;
    o->sec_off[i] = off;
    if (dev) {
      // host sections lying between two device sections of one round are
      // holes in the arena: the span test below accounts for them
      const int32_t g = group ? group[i] : 0;
      if (o->round_lo.empty() || g != cur_group ||
          off + len - o->round_lo.back() > arena_bytes) {
        cur_group = g;
        o->round_lo.push_back(off);
        o->round_hi.push_back(off);
      }
      o->round[i] = (int32_t)o->round_lo.size() - 1;
      o->round_hi.back() = off + len;
    }
    off += len;
  }
  o->required = off;
  return off > cap ? P_ENOBUF : P_OK;
}

// u32 n and the directory (the caller has checked required <= cap); the
// sections themselves are written elsewhere
inline void WriteDirectory(uint8_t* out, const int32_t* status,
                           const int32_t* more, uint64_t header_rev, size_t n,
                           const PlanOut& o) {
  uint32_t n32 = (uint32_t)n;
  memcpy(out, &n32, 4);
  for (size_t i = 0; i < n; ++i) {
    uint8_t* p = out + 4 + kDirEntry * i;
    memcpy(p, &status[i], 4);
    memcpy(p + 4, &more[i], 4);
    memcpy(p + 8, &header_rev, 8);
    memcpy(p + 16, &o.len[i], 8);
  }
}

}  // namespace kblist
