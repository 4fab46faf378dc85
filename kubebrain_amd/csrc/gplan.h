// kubebrain_amd/csrc/gplan.h — pure host half of the batched point read
// (kb_get_batch): the reply planner and the emit-round
// splitter. No HIP calls and no store state, so CPU tests (kb_test_get_plan)
// and a stand-alone sanitizer build can exercise it without a GPU.
#pragma once

#include <cstdint>
#include <vector>

namespace kbget {

// status codes used by the planner (== include/kb_slab.h kb_status)
constexpr int P_OK = 0, P_EINVALID = 5, P_ENOBUF = 100;

// reply = u32 n; n x DirEntry; then the value bytes of every has_kv entry,
// back to back in query order
constexpr uint64_t kDirEntry = 32;  // i32 status; i32 has_kv; u64 header_rev;
                                    // u64 mod_rev; u64 vlen

constexpr int32_t R_NONE = -1;  // no value bytes (not found, tombstone, vlen 0)
constexpr int32_t R_HOST = -2;  // one value larger than the arena: host path

struct PlanOut {
  std::vector<uint64_t> val_off;  // reply offset of each query's value bytes
  std::vector<int32_t> round;     // emit round, R_NONE or R_HOST
  // per emit round the queries [lo, hi) it launches over: lo and hi - 1 carry
  // value bytes, queries without bytes may lie between them
  std::vector<uint64_t> round_lo, round_hi;
  uint64_t required = 4;
  uint64_t found = 0;   // has_kv entries
  uint64_t n_host = 0;  // R_HOST entries
};

// Queries i / max_q form one sub-batch. A round is a maximal run of
// consecutive queries of one sub-batch whose value bytes together fit
// arena_bytes: the run ends at the sub-batch's end, before a host-path query
// and before the query that would overflow the arena. vlen of a query
// without has_kv must be 0 (P_EINVALID otherwise, as for max_q == 0).
inline int Plan(const int32_t* has_kv, const uint64_t* vlen, size_t n,
                size_t max_q, uint64_t cap, uint64_t arena_bytes, PlanOut* o) {
  o->val_off.assign(n, 0);
  o->round.assign(n, R_NONE);
  o->round_lo.clear();
  o->round_hi.clear();
  o->required = 4;
  o->found = 0;
  o->n_host = 0;
  if (max_q == 0) return P_EINVALID;
  uint64_t off = 4 + kDirEntry * (uint64_t)n;
  bool open = false;    // a round is open and may take more queries
  uint64_t fill = 0;    // value bytes of the open round
  for (size_t i = 0; i < n; ++i) {
    if (i % max_q == 0) open = false;
    o->val_off[i] = off;
    if (!has_kv[i]) {
      if (vlen[i] != 0) return P_EINVALID;
      continue;
    }
    o->found++;
    const uint64_t len = vlen[i];
    if (len == 0) continue;
    if (len > arena_bytes) {
      o->round[i] = R_HOST;
      o->n_host++;
      open = false;
    } else {
      if (!open || len > arena_bytes - fill) {
        o->round_lo.push_back(i);
        o->round_hi.push_back(i);
        open = true;
        fill = 0;
      }
      o->round[i] = (int32_t)o->round_lo.size() - 1;
      o->round_hi.back() = i + 1;
      fill += len;
    }
    off += len;
  }
  o->required = off;
  return off > cap ? P_ENOBUF : P_OK;
}

}  // namespace kbget
