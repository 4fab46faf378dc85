// kubebrain_amd/csrc/slab_dev.h — host-visible interface of the HBM slab
// engine (implemented in slab.hip, gfx950 kernels). PRODUCT code: no CPU
// fallback; creation fails without a HIP device.
//
// Data model: one sorted columnar run in HBM, ordered by
// (userKey, rev) == the reference's internal-key order
// (coder/normal.go:42-50), plus an append-only value heap.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace kbslab {

constexpr int KEYW = 96;  // fixed-width zero-padded key column
// Keys LONGER than KEYW (SURVEY §7 hard part (a)): the column holds the
// first 96 bytes; the tail lives in an append-only key-spill heap addressed
// by the per-row `ko` column. Ordering: the zero-padded 96B prefix decides
// every compare except exact 96-byte prefix ties (impossible unless both
// keys are >= 96B, since key bytes are > 0x24 > 0x00), which compare tails.
constexpr int KB_MAX_KEY = 4096;  // validated bound (meta klen is 16-bit)

// meta word bits (per row)
constexpr uint64_t M_SAME_NEXT = 1ull << 0;  // next row has the same user key
constexpr uint64_t M_TOMB = 1ull << 1;       // value == "tombstone" (util.go:28)
constexpr uint64_t M_FLAG9 = 1ull << 2;      // 9-byte revision value (rev.go:26)
constexpr uint64_t M_EVENTS = 1ull << 3;     // key contains "/events/" (TTL)

#ifdef __HIPCC__
#define KB_HD __host__ __device__
#else
#define KB_HD
#endif
KB_HD inline uint64_t meta_make(bool tomb, bool flag9, bool events,
                                uint32_t klen, uint32_t vlen) {
  return (tomb ? M_TOMB : 0) | (flag9 ? M_FLAG9 : 0) | (events ? M_EVENTS : 0) |
         ((uint64_t)(klen & 0xffff) << 16) | ((uint64_t)vlen << 32);
}
KB_HD inline uint32_t meta_klen(uint64_t m) { return (uint32_t)((m >> 16) & 0xffff); }
KB_HD inline uint32_t meta_vlen(uint64_t m) { return (uint32_t)(m >> 32); }

#pragma pack(push, 1)
struct DevRangeQ {
  uint8_t start[KEYW];
  uint8_t end[KEYW];
  // true bound lengths; tails of bounds longer than KEYW live in the
  // per-batch query-tail buffer at start_ko/end_ko
  uint32_t start_klen, end_klen;
  uint64_t start_ko, end_ko;
  uint64_t read_rev;
  // scan begins at the first row with (key,rev) >= (start, start_rev).
  // 0 = inclusive start-of-key (the normal case); UINT64_MAX = strictly
  // after every row of `start` — the exclusive continuation bound chunked
  // List/Stream use (exact even for keys of the full KEYW width, where a
  // key-suffix trick would truncate)
  uint64_t start_rev;
  int64_t cap;        // winner-write cap per query (limit+1); <=0 => unbounded
  int32_t count_only;
  // etcd3 RangeRequest.KeysOnly semantics (an extension: the reference's etcd
  // shim ignores the flag, kv.go:48-67): gather key + mod-revision per winner,
  // no value bytes (header vlen = 0)
  int32_t keys_only;
};
struct DevGetQ {
  uint8_t key[KEYW];
  uint32_t klen, _pad;  // true key length; tail at ko when > KEYW
  uint64_t ko;
  uint64_t read_rev;  // UINT64_MAX for "latest"
};
#pragma pack(pop)
// the step staging block's layout (stepstage.h) is checked at these sizes
static_assert(sizeof(DevRangeQ) == 248 && sizeof(DevGetQ) == 120,
              "device query layout");

struct RangeResult {
  int64_t written = 0;   // winners materialized (<= cap)
  int64_t total = 0;     // winners seen before stop (exact when unbounded)
  int64_t bytes = 0;     // gathered record bytes for this query
  bool overflow = false; // per-query arena too small; retry with bigger qcap
  // parsed records (filled only in d2h mode): {rev, key, val}
  struct Rec { uint64_t rev; std::string key, val; };
  std::vector<Rec> recs;
};

struct GetResult {
  bool found = false;
  bool tomb = false;
  uint64_t rev = 0;
  uint32_t vlen = 0;  // value length (filled even in meta-only mode)
  std::string val;
};

// sorted delta (memtable flush) — vo entries already ABSOLUTE heap offsets
// (host adds the pre-merge heap_used base) or objRev for rev rows.
struct DeltaRows {
  std::vector<uint8_t> keys;  // m * KEYW (96B zero-padded prefixes)
  std::vector<uint64_t> meta, rev, vo;
  std::vector<uint64_t> ko;   // spill offsets for keys > KEYW (empty = none)
  std::vector<uint8_t> heap;  // new value bytes (4B-aligned records)
  int64_t m = 0;
};

struct DumpRow {
  std::string key;  // user key
  uint64_t rev;
  uint64_t meta;
  std::string val;  // object rows: heap bytes; rev rows: empty (vo=objRev)
  uint64_t vo;
};

struct Perf {
  double scan_ms = 0, gather_ms = 0, get_ms = 0, compact_ms = 0, merge_ms = 0,
         filter_ms = 0, pack_d2h_ms = 0;
  int64_t scan_launches = 0, gather_launches = 0, get_launches = 0,
          merges = 0, compacts = 0, filter_launches = 0;
  int64_t rows_scanned = 0, bytes_gathered = 0, winners = 0,
          filter_events = 0, filter_watchers = 0;
  double dbg_a = 0, dbg_b = 0, dbg_c = 0, dbg_d = 0, dbg_e = 0;
  // batched watch poll (kb_watch_poll_batch): k_wpoll_size + k_wpoll_emit
  // kernel time, the reply D2H, events served per path, device bytes moved
  double wpoll_ms = 0, wpoll_d2h_ms = 0;
  int64_t wpoll_launches = 0, wpoll_events_dev = 0, wpoll_events_host = 0,
          wpoll_bytes = 0;
  // batched List (kb_list_batch): k_list_size + k_list_emit kernel time, the
  // section D2H, queries per path, kvs and device bytes moved
  double list_ms = 0, list_d2h_ms = 0;
  int64_t list_batch_calls = 0, list_batch_q_dev = 0, list_batch_q_host = 0,
          list_batch_kvs = 0, list_batch_bytes = 0, list_emit_launches = 0;
  // batched point read (kb_get_batch): k_get_find + k_get_plan + k_get_emit
  // kernel time, the directory and value D2H, queries per path, entries with
  // a kv, value bytes moved from the arena, three-kernel launches
  double get_batch_ms = 0, get_batch_d2h_ms = 0;
  int64_t get_batch_calls = 0, get_batch_q_dev = 0, get_batch_q_host = 0,
          get_batch_found = 0, get_batch_bytes = 0, get_batch_launches = 0;
  // batched Count (kb_count_batch): k_count_plan + k_count_tiles kernel time,
  // the counter D2H, queries the kernels served, launches, tiles counted and
  // rows covered by them (= sum of the segment lengths)
  double count_ms = 0, count_d2h_ms = 0;
  int64_t count_batch_calls = 0, count_batch_q = 0, count_batch_launches = 0,
          count_batch_tiles = 0, count_batch_rows = 0;
  // which mergeRuns branch ran (k_merge_small / k_delta_rank + k_delta_scatter /
  // k_merge_rank_inv_big / the n == 0 scatter), delta appends that took the
  // async no-sync branch, and delta->base folds: the tests prove with these
  // that a workload reached the path it claims to cover
  int64_t merge_small = 0, merge_insert = 0, merge_big = 0, merge_empty = 0,
          merges_async = 0, folds = 0;
};

// batched watch poll: one delivery bitmap reference (<= 512 events of the
// event ring starting at sequence `base`) of the watcher at index widx of
// the call's wids[]
struct WpollRef {
  int64_t base;
  int32_t count;
  int32_t widx;
  uint64_t words[8];
};
static_assert(sizeof(WpollRef) == 80, "ref table entry layout");
// k_wpoll_size result per ref
struct WpollSize {
  uint64_t bytes;
  uint32_t count;
  uint32_t _pad;
};
// one contiguous piece of a payload push: staging bytes -> byte-ring offset
struct PaySeg { int64_t ring_off, stage_off, len; };
// batched List (kb_list_batch): k_list_size result per query
struct ListSize {
  uint64_t bytes;  // wire bytes of the records (without the u32 count)
  uint32_t count;  // records = min(found, limit)
  uint32_t flags;  // LS_MORE | LS_PARTIAL
};
constexpr uint32_t LS_MORE = 1;     // kb_list's `more` (found > limit)
constexpr uint32_t LS_PARTIAL = 2;  // the winner table did not hold the whole
                                    // answer: the host path must serve it
static_assert(sizeof(ListSize) == 16, "list size entry layout");
// batched point read (kb_get_batch): what k_get_plan leaves per launch. The
// entries are the reply's directory entries in wire form.
struct GetDirEntry {
  int32_t status, has_kv;
  uint64_t header_rev, mod_rev, vlen;
};
struct GetBatchHdr {
  uint64_t total;    // value bytes of the launch = extent of its arena layout
  uint64_t skipped;  // queries k_get_emit did not copy (no bytes, or unsafe)
  GetDirEntry dir[1];  // nq entries
};
static_assert(sizeof(GetDirEntry) == 32, "get directory entry layout");
static_assert(sizeof(GetBatchHdr) == 48, "get launch header layout");
// batched Count (kb_count_batch): what k_count_plan and k_count_tiles leave
// per launch. tiles / rows are what the tile kernel covered, *_planned what
// the plan kernel derived from the bounds; they must agree.
struct CountBatchHdr {
  uint64_t tiles, rows, tiles_planned, rows_planned;
  uint64_t count[1];  // nq entries
};



class Slab {
 public:
  // device < 0: use current device. Returns nullptr + *err on failure
  // (including "no HIP device": the product path fails loudly).
  static Slab* Create(int64_t max_rows, int64_t heap_cap, int device,
                      std::string* err);
  ~Slab();

  int64_t rows() const;
  int64_t delta_rows() const;
  int64_t delta_capacity() const;
  int64_t heap_used() const;
  // per-query winner cap of the device arena (KB_MAX_CAP); chunked List
  // clamps each chunk's cap to this and continues the frontier loop
  int64_t max_winner_cap() const;

  // merge sorted delta rows straight into the BASE run (GPU merge by ranks;
  // delta rev-rows REPLACE base rev-rows of the same key). Used by tests and
  // bulk paths; the hot write path uses AppendRows/Fold below.
  bool Merge(const DeltaRows& d, std::string* err);

  // append value bytes to the device heap; *off = absolute offset
  bool HeapAppend(const void* p, int64_t len, int64_t* off, std::string* err);
  // append key-tail bytes to the key-spill heap (keys > KEYW); *off absolute
  bool SpillAppend(const void* p, int64_t len, int64_t* off, std::string* err);
  int64_t spill_used() const;
  // merge sorted new rows (vo already absolute) into the DELTA run.
  // known_new_dn >= 0: the caller knows the exact post-merge row count
  // (drops = rev-row replacements it tracked), so the merge runs fully
  // async — no host sync; the next kernel on the stream queues behind it.
  // KB_VALIDATE_DN=1 re-checks the prediction (enabled by the test env).
  bool AppendRows(const uint8_t* keys, const uint64_t* meta, const uint64_t* rev,
                  const uint64_t* vo, const uint64_t* ko, int64_t m,
                  std::string* err, int64_t known_new_dn = -1);
  // the same without the intermediate vectors: BeginRowUpload hands out the
  // five column slices of a pinned mirror (stride m, stepstage.h PlanRows),
  // the caller writes its m sorted rows into them, CommitRowUpload queues
  // ONE H2D of the span and the merge. AppendRows is Begin + memcpy + Commit.
  struct RowUpload { uint8_t* keys; uint64_t *meta, *rev, *vo, *ko; };
  bool BeginRowUpload(int64_t m, RowUpload* u, std::string* err);
  bool CommitRowUpload(int64_t m, std::string* err, int64_t known_new_dn = -1);
  // fold the delta run into the base run; delta becomes empty
  bool Fold(std::string* err);

  // batched Range (the north-star kernel; scanner worker.run semantics,
  // scanner.go:389-516). d2h=false leaves records in the device arena
  // (bench "value" mode); d2h=true packs + copies + parses them.
  // qtails = concatenated tails of bounds longer than KEYW (may be empty)
  bool RangeBatch(const std::vector<DevRangeQ>& qs, bool d2h,
                  std::vector<RangeResult>* outs, std::string* err,
                  const std::string& qtails = std::string());
  // parse=false: D2H into pinned memory without materializing records
  bool RangeBatchEx(const std::vector<DevRangeQ>& qs, bool d2h, bool parse,
                    std::vector<RangeResult>* outs, std::string* err,
                    const std::string& qtails = std::string());
  // async split: Start launches the scan+gather without syncing, so host
  // work (e.g. the txn leg) overlaps the in-flight kernels; Finish collects.
  // d2h with parse=false runs PIPELINED: the payload copy lands in pinned
  // host memory on a copy stream, overlapping the next batch's kernels —
  // call DrainD2H() before reading wall-clock results.
  bool RangeBatchStart(const std::vector<DevRangeQ>& qs, std::string* err,
                       const std::string& qtails = std::string());
  // Start also queues the batch's counter read-back into one of two pinned
  // mirrors and records that slot's "results ready" event; range_slot() names
  // the slot of the batch started last. Finish waits on its slot's event
  // only, never on the stream, so batch i+1 may be started before batch i is
  // finished (slot = the value range_slot() returned after batch i's Start;
  // -1 = the batch started last). Only the counters are per slot: d2h needs
  // the arena and therefore the latest batch.
  bool RangeBatchFinish(int nq, bool d2h, bool parse,
                        std::vector<RangeResult>* outs, std::string* err,
                        int slot = -1);
  int range_slot() const;
  bool DrainD2H(std::string* err);
  // step staging block (stepstage.h): the get queries, range queries and key
  // tails of one bench step go up in ONE H2D. Begin returns where to write
  // nget + nrange queries and up to tail_cap tail bytes (pinned, double
  // buffered; the ko offsets of both query kinds index the one tail slice).
  // Commit queues the upload of the used span; the two Staged starts then
  // launch over the staged slices exactly like GetBatchStart and
  // RangeBatchStart (finish them with GetBatchFinish / RangeBatchFinish).
  struct StepStage { DevGetQ* gq; DevRangeQ* rq; uint8_t* tails; int64_t tail_cap; };
  bool StepStageBegin(int nget, int nrange, StepStage* st, std::string* err);
  bool StepStageCommit(int64_t tail_bytes, std::string* err);
  bool GetBatchStartStaged(std::string* err);
  bool RangeBatchStartStaged(std::string* err);
  // batched List (kb_list_batch). RangeScanStart is the scan
  // half of RangeBatchStart alone (k_range_bounds + k_range_scan2): tagged
  // winner rows per query, no gather. ListSizeBatch runs it, then k_list_size
  // (per-winner wire offsets into the offsets scratch, per-query ListSize)
  // and reads back 16 B per query; *sizes points into pinned memory valid
  // until the next call. The sized sub-batch stays resident for ListEmit.
  int max_queries() const;     // KB_MAX_Q
  int64_t arena_bytes() const; // KB_ARENA_BYTES: bounds one emit round
  bool RangeScanStart(const std::vector<DevRangeQ>& qs, std::string* err,
                      const std::string& qtails = std::string());
  bool ListSizeBatch(const std::vector<DevRangeQ>& qs,
                     const std::string& qtails, const ListSize** sizes,
                     std::string* err);
  // pinned reply buffer of >= total bytes; contents survive until the next
  // call with a larger total
  uint8_t* ListReply(int64_t total, std::string* err);
  // pinned per-query emit plan the host fills in place: base[max_q] = arena
  // offset of a query's first record, cum[max_q+1] = records emitted before
  // query q in this round (a query outside the round adds none)
  bool ListPlanStaging(uint64_t** base, uint64_t** cum, std::string* err);
  // one emit round over the resident sub-batch: k_list_emit writes the
  // staged queries' records into the arena, then arena [0, span) arrives at
  // reply + reply_off with one D2H
  bool ListEmit(int nq, int64_t span, uint8_t* reply, int64_t reply_off,
                std::string* err);
  // kb_test_last_range reports an empty batch from here on (the arena no
  // longer holds gathered records)
  void ForgetLastRange();
  // TEST HOOK (kb_test_last_range): the records of the most recent
  // RangeBatchFinish in the wire format documented in include/kb_slab.h.
  // src 0 reads each query's region of the device arena, src 1 the pinned
  // buffer the pipelined D2H of that batch filled. Launches no kernel.
  bool LastRangeWire(int src, std::string* wire, std::string* err);

  // batched MVCC point read (range.go:91-121 reverse-iter semantics).
  // GetBatchEx(values=false) skips the value copy (meta-only: found/rev/
  // tomb) — the device-side revIndex lookup of the batched txn path.
  bool GetBatch(const std::vector<DevGetQ>& qs, std::vector<GetResult>* outs,
                std::string* err,
                const std::string& qtails = std::string());
  bool GetBatchEx(const std::vector<DevGetQ>& qs, bool values,
                  std::vector<GetResult>* outs, std::string* err,
                  const std::string& qtails = std::string());
  // async split: Start launches the lookup; Finish waits ONLY on the
  // lookup's completion event, so kernels launched on the stream AFTER
  // Start (e.g. the range batch) keep running while the host consumes the
  // results. values=false only (meta-only lookups).
  bool GetBatchStart(const std::vector<DevGetQ>& qs, std::string* err,
                     const std::string& qtails = std::string());
  bool GetBatchFinish(int nq, std::vector<GetResult>* outs, std::string* err);
  // batched point read with values (kb_get_batch).
  // GetBatchLaunch uploads nq <= KB_MAX_Q queries and runs k_get_find,
  // k_get_plan and (unless no_values) k_get_emit back to back, then reads
  // back {total, skipped, nq directory entries}; *hdr points into pinned
  // memory valid until the next call. The values of the launch lie packed in
  // query order from arena offset 0, as far as the arena reaches.
  bool GetBatchLaunch(const DevGetQ* qs, int nq, const std::string& qtails,
                      bool no_values, uint64_t committed,
                      const GetBatchHdr** hdr, std::string* err);
  // arena [0, span) of the resident launch -> reply + reply_off, one D2H;
  // reply is the pinned buffer of ListReply
  bool GetBatchFetch(int64_t span, uint8_t* reply, int64_t reply_off,
                     std::string* err);
  // host path for one value the arena cannot hold: k_get_find for the query
  // alone, then a plain D2H of its vlen heap bytes to dst. Fails if the row
  // is not the (mod_rev, vlen) the batch's directory reported. Displaces the
  // resident launch.
  bool GetBatchHostValue(const DevGetQ& q, const std::string& qtails,
                         uint64_t mod_rev, uint64_t vlen, uint8_t* dst,
                         std::string* err);

  // batched Count (kb_count_batch). CountBatchLaunch uploads
  // nq <= KB_MAX_Q queries (read_rev resolved; start_rev, cap and the flags
  // are not read) and runs k_range_bounds, k_count_plan and k_count_tiles
  // back to back on buffers of its own, then reads back the totals and 8 B
  // per query; *hdr points into pinned memory valid until the next call.
  // Writes neither the winner tables nor the arena nor the range counters.
  bool CountBatchLaunch(const DevRangeQ* qs, int nq, const std::string& qtails,
                        const CountBatchHdr** hdr, std::string* err);
  int64_t count_tile() const;  // KB_COUNT_TILE: rows per tile

  // compaction mark+sweep over encoded borders (compact.go:55-68 +
  // scanner.go:444-491, 566-591). Bounds are (key96, rev) pairs.
  // timeout_revs[i] is the TTL timeout revision of border pair i — the
  // reference pops one per scanner.Compact scan (scanner.go:147-177), so
  // with >=2 pairs the values differ per pair.
  struct Bound { uint8_t key[KEYW]; uint64_t rev; };
  bool Compact(const std::vector<std::pair<Bound, Bound>>& borders,
               uint64_t compact_rev, const std::vector<uint64_t>& timeout_revs,
               std::string* err);

  // full slab dump for parity diffs (debug; D2H of all columns + used heap)
  bool Dump(std::vector<DumpRow>* rows_out, std::string* err);

  // device-resident event log (north_star: GPU-resident event log): ring of
  // (key96, rev) columns pushed once per event batch; the fan-out filter and
  // catch-up scans read the resident ring. Values/full events stay host-side
  // for materialization at poll time.
  bool EventRingInit(int64_t cap, std::string* err);
  bool EventRingPush(const uint8_t* keys96, const uint64_t* revs,
                     int64_t count, int64_t base_seq, std::string* err);
  // fan-out: bitmap[w][ceil(count/64)] over all registered watchers for the
  // ring span [base_seq, base_seq+count)
  bool WatchFilterRing(int64_t base_seq, int64_t count,
                       std::vector<uint64_t>* bitmap, int64_t* n_watch_slots,
                       std::string* err);
  // catch-up: one prefix/from_rev filter over a resident ring span
  bool WatchCatchup(const uint8_t* pfx96, uint32_t plen, uint64_t from_rev,
                    int64_t base_seq, int64_t count,
                    std::vector<uint64_t>* words_out, std::string* err);
  // device payload ring: per-event er_poff/er_plen columns
  // next to (key96, rev) plus a byte ring holding each event in wire form.
  // Allocated by PayloadArm (first kb_watch_poll_batch); placement is the
  // host's (wpoll.h PayRing). PayloadStaging returns pinned memory the host
  // serializes into; PayloadPush copies its segments to the ring and the
  // column entries for [base_seq, base_seq+count) on the store's stream.
  bool PayloadArm(int64_t ring_bytes, std::string* err);
  uint8_t* PayloadStaging(int64_t need, std::string* err);
  bool PayloadPush(const PaySeg* segs, size_t nsegs, const uint64_t* poffs,
                   const uint32_t* plens, int64_t count, int64_t base_seq,
                   std::string* err);
  // batched poll: pinned ref table / per-ref destination offsets the host
  // fills in place (grown on demand; contents are not preserved on growth)
  WpollRef* WpollRefStaging(int64_t nrefs, std::string* err);
  uint64_t* WpollOffStaging(int64_t nrefs, std::string* err);
  // upload the ref table, run k_wpoll_size, read back 16 B per ref (the
  // result points into pinned memory valid until the next call)
  bool WpollSizeRefs(int64_t nrefs, const WpollSize** sizes, std::string* err);
  // run k_wpoll_emit for the uploaded refs with the staged offsets: records
  // land in a device arena laid out like the reply; bytes [lo, hi) then
  // arrive in the pinned reply buffer (>= total bytes) with one D2H copy
  bool WpollEmit(int64_t nrefs, int64_t lo, int64_t hi, int64_t total,
                 uint8_t** reply, std::string* err);

  bool WatcherSet(int64_t slot, const uint8_t* prefix, uint32_t plen,
                  uint64_t from_rev, std::string* err);  // slot grows table
  void WatcherClear(int64_t slot);

  Perf perf;

  struct Impl;
  Impl* p;

 private:
  bool launchScan(int nq, std::string* err);
  bool launchGather(const DevRangeQ* hq, int nq, std::string* err);
  bool launchGet(int nq, std::string* err);
};

}  // namespace kbslab
