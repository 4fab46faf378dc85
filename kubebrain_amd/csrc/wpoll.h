// kubebrain_amd/csrc/wpoll.h — pure host half of the batched watch poll
// (kb_watch_poll_batch): the wire-record serializer, the
// payload byte-ring placement and the reply planner. No HIP calls and no
// store state, so CPU tests (kb_test_wpoll_plan) and a stand-alone sanitizer
// build can exercise it without a GPU.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace kbwpoll {

// status codes used by the planner (== include/kb_slab.h kb_status)
constexpr int P_OK = 0, P_EINVALID = 5, P_EINTERNAL = 13, P_ENOBUF = 100;

// one event in kb_watch_poll wire form:
// i32 type | u64 rev | u64 kv_rev | u32 klen | key | u32 vlen | val
inline size_t RecordSize(size_t klen, size_t vlen) { return 28 + klen + vlen; }

inline uint8_t* PutRecord(uint8_t* p, int32_t type, uint64_t rev,
                          uint64_t kv_rev, const void* key, uint32_t klen,
                          const void* val, uint32_t vlen) {
  memcpy(p, &type, 4); p += 4;
  memcpy(p, &rev, 8); p += 8;
  memcpy(p, &kv_rev, 8); p += 8;
  memcpy(p, &klen, 4); p += 4;
  if (klen) memcpy(p, key, klen);
  p += klen;
  memcpy(p, &vlen, 4); p += 4;
  if (vlen) memcpy(p, val, vlen);
  return p + vlen;
}

// ---- payload byte ring placement ---------------------------------------
// Records start 16-byte aligned and never straddle the wrap point. The ring
// is a FIFO: placing a record evicts the oldest resident records it
// overlaps (and, when it wraps to offset 0, everything left in the skipped
// tail). `oldest_seq` is the oldest event sequence whose bytes are resident.
struct PayRing {
  int64_t cap = 0;         // bytes, multiple of 16
  int64_t head = 0;        // next write offset
  int64_t oldest_seq = 0;  // resident window = [oldest_seq, next seq)
  int64_t slots = 0;       // event-ring capacity (mirror size)
  std::vector<uint64_t> poff;   // [slots] placement of seq % slots
  std::vector<uint32_t> alen;   // [slots] aligned length (0 = not resident)

  void init(int64_t cap_bytes, int64_t event_slots, int64_t first_seq) {
    cap = cap_bytes & ~(int64_t)15;
    head = 0;
    oldest_seq = first_seq;
    slots = event_slots;
    poff.assign((size_t)slots, 0);
    alen.assign((size_t)slots, 0);
  }
  void evict(int64_t lo, int64_t hi, int64_t seq) {
    while (oldest_seq < seq) {
      size_t s = (size_t)(oldest_seq % slots);
      int64_t a = (int64_t)poff[s], b = a + (int64_t)alen[s];
      if (alen[s] != 0 && (b <= lo || a >= hi)) break;
      ++oldest_seq;
    }
  }
  // place event `seq` (wire length len); returns its ring offset, or -1
  // when the record is larger than the whole ring (window emptied up to and
  // including seq)
  int64_t place(int64_t seq, uint64_t len) {
    size_t s = (size_t)(seq % slots);
    // mirror slots older than the event-ring window are about to be reused
    if (oldest_seq < seq + 1 - slots) oldest_seq = seq + 1 - slots;
    uint64_t al = (len + 15) & ~(uint64_t)15;
    if (al > (uint64_t)cap || al > 0xfffffff0ull) {
      oldest_seq = seq + 1;
      poff[s] = 0;
      alen[s] = 0;
      return -1;
    }
    if (head + (int64_t)al > cap) {
      evict(head, cap, seq);
      head = 0;
    }
    evict(head, head + (int64_t)al, seq);
    poff[s] = (uint64_t)head;
    alen[s] = (uint32_t)al;
    int64_t at = head;
    head += (int64_t)al;
    return at;
  }
};

// ---- reply planner --------------------------------------------------------
// reply = u32 n; n x { i32 status; u32 len; len bytes } in watcher order.
// A section with status OK is u32 count + its records; any other status has
// len 0. host_len[i] >= 4 gives the size of a section the host serializes;
// host_len[i] < 0 marks a device-path watcher whose size is 4 + the bytes of
// its refs (refs arrive in watcher order).
struct PlanRef { uint64_t bytes; uint32_t count; int32_t widx; };
struct PlanOut {
  std::vector<uint32_t> len, count;   // per watcher (count: device path only)
  std::vector<uint64_t> sec_off;      // per watcher: offset of its len bytes
  std::vector<uint64_t> ref_off;      // per ref: offset of its first record
  uint64_t required = 4;
  uint64_t dev_lo = 0, dev_hi = 0;    // byte span holding every device record
};

inline int Plan(const PlanRef* refs, size_t nrefs, const int32_t* status,
                const int64_t* host_len, size_t n, uint64_t cap,
                PlanOut* o) {
  o->len.assign(n, 0);
  o->count.assign(n, 0);
  o->sec_off.assign(n, 0);
  o->ref_off.assign(nrefs, 0);
  o->dev_lo = o->dev_hi = 0;
  uint64_t off = 4;
  size_t r = 0;
  for (size_t i = 0; i < n; ++i) {
    off += 8;  // status + len
    o->sec_off[i] = off;
    uint64_t len = 0;
    if (status[i] == P_OK && host_len[i] >= 0) {
      if (host_len[i] < 4) return P_EINVALID;
      len = (uint64_t)host_len[i];
    } else if (status[i] == P_OK) {
      len = 4;
      uint64_t cnt = 0;
      for (; r < nrefs && refs[r].widx == (int32_t)i; ++r) {
        o->ref_off[r] = off + len;
        if (refs[r].bytes) {
          if (o->dev_hi == 0) o->dev_lo = off + len;
          o->dev_hi = off + len + refs[r].bytes;
        }
        len += refs[r].bytes;
        cnt += refs[r].count;
      }
      if (cnt > 0xffffffffull) return P_EINTERNAL;
      o->count[i] = (uint32_t)cnt;
    }
    // a ref that belongs to an earlier, a non-OK or a host-path watcher
    if (r < nrefs && (refs[r].widx < 0 || (size_t)refs[r].widx <= i))
      return P_EINVALID;
    if (len > 0xffffffffull) return P_EINTERNAL;  // u32 len field
    o->len[i] = (uint32_t)len;
    off += len;
  }
  if (r != nrefs) return P_EINVALID;
  o->required = off;
  return off > cap ? P_ENOBUF : P_OK;
}

// directory + per-watcher header fields into the reply buffer (the caller
// has checked required <= cap); sections themselves are written elsewhere
inline void WriteDirectory(uint8_t* out, const int32_t* status, size_t n,
                           const PlanOut& o) {
  uint32_t n32 = (uint32_t)n;
  memcpy(out, &n32, 4);
  for (size_t i = 0; i < n; ++i) {
    uint8_t* p = out + o.sec_off[i] - 8;
    memcpy(p, &status[i], 4);
    memcpy(p + 4, &o.len[i], 4);
  }
}

}  // namespace kbwpoll
