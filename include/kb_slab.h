/* include/kb_slab.h — the drop-in C-ABI boundary of the MI355X-native
 * KubeBrain MVCC hot path (libkbslab.so).
 *
 * Every entry point cites the reference interface it replaces (paths into
 * /root/reference). A Go host binds this behind `storage.KvStorage` +
 * backend fast-path dispatch via cgo (see INTEGRATION.md for the binding
 * stub); error codes mirror the Go error taxonomy
 * (pkg/storage/interface.go:140-147, errors.go:20-70).
 *
 * Threading: all calls are thread-safe; writes are internally serialized
 * (single-writer, matching leader-only writes, pkg/server/etcd/kv.go:90-96).
 * Ownership: callers own all out buffers; the library copies in/out (the
 * reference's iterators copy too, pkg/storage/badger/iter.go:85-92).
 *
 * The library REQUIRES a HIP device (MI355X/gfx950): kb_new returns NULL and
 * kb_last_error() reports KB_ENOGPU when none is present. There is no CPU
 * fallback.
 */
#ifndef KB_SLAB_H
#define KB_SLAB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes (== oracle/oracle.h codes; mirror storage/interface.go:140-147) */
enum kb_status {
  KB_OK = 0,
  KB_ENOTFOUND = 1,     /* storage.ErrKeyNotFound */
  KB_ECAS_FAILED = 2,   /* storage.ErrCASFailed */
  KB_EUNCERTAIN = 3,    /* storage.ErrUncertainResult (unreachable: local engine) */
  KB_ECOMPACTED = 4,    /* range revision < compact revision (scanner.go:617-621) */
  KB_EINVALID = 5,      /* invalid nil end / invalid range end (range.go:139-151) */
  KB_EUNSUPPORTED = 6,  /* ListByStream/GetPartitions: SURVEY.md §8f3, round-2+ */
  KB_EREV_DRIFT = 7,    /* backend.ErrRevisionDriftBack (backend.go:188) */
  KB_EWATCH_LOW = 8,    /* "cache event oldest revision ... newer" (watch.go:79-84) */
  KB_EWATCH_EMPTY = 9,  /* "empty cache event" (watch.go:67-71) */
  KB_EWATCH_DROPPED = 10, /* slow consumer dropped (watcherhub.go:84-94) */
  KB_EKEYTOOLONG = 11,  /* key > 96B: documented round-1 limit */
  KB_EBADKEY = 12,      /* key byte <= 0x24: the reference codec itself mis-orders
                           such keys (coder/normal.go:29-31) */
  KB_EINTERNAL = 13,
  KB_ENOGPU = 14,       /* no HIP device — the product path never falls back */
  KB_ENOBUF = 100       /* caller buffer too small; retry with a larger one */
};

typedef struct kb_store kb_store; /* one MVCC store on one GPU */

/* ---- lifecycle ----
 * Replaces backend.NewBackend wiring (pkg/backend/backend.go:145-186).
 * Capacity knobs via env: KB_MAX_ROWS (default 8M), KB_HEAP_BYTES (default
 * 2G), KB_FLUSH_ROWS (memtable flush threshold, default 65536), KB_DEVICE.
 */
kb_store* kb_new(const char* prefix, int watch_cache_size,
                 long long events_ttl_seconds, int enable_etcd_compatibility);
void kb_free(kb_store*);
int kb_last_error(char* msg, size_t cap); /* returns last kb_status, fills message */

/* ---- writes (leader txn protocol) ---- */
/* backend.Create (txn.go:33-77, creator/naive.go:48-105) */
int kb_create(kb_store*, const uint8_t* key, size_t klen, const uint8_t* val,
              size_t vlen, uint64_t* header_rev, int* succeeded);
/* backend.Update (txn.go:193-265); prev_rev==0 => create path */
int kb_update(kb_store*, const uint8_t* key, size_t klen, const uint8_t* val,
              size_t vlen, uint64_t prev_rev, uint64_t* header_rev, int* succeeded,
              int* has_kv, uint8_t* kv_val, size_t cap, size_t* kv_val_len,
              uint64_t* kv_rev);
/* backend.Delete (txn.go:79-190) */
int kb_delete(kb_store*, const uint8_t* key, size_t klen, uint64_t prev_rev,
              uint64_t* header_rev, int* succeeded, int* has_kv, uint8_t* kv_val,
              size_t cap, size_t* kv_val_len, uint64_t* kv_rev);

/* ---- reads (the GPU hot path) ---- */
/* backend.Get (range.go:34-121): MVCC point read at revision (0 = latest) */
int kb_get(kb_store*, const uint8_t* key, size_t klen, uint64_t rev,
           uint64_t* header_rev, int* has_kv, uint8_t* val, size_t cap,
           size_t* vlen, uint64_t* mod_rev);
/* backend.List (range.go:124-174): out = packed records
 * {u32 n; n × {u64 rev; u32 klen; key; u32 vlen; val}} (same wire as oracle) */
int kb_list(kb_store*, const uint8_t* start, size_t slen, const uint8_t* end,
            size_t elen, uint64_t rev, int64_t limit, uint8_t* out, size_t cap,
            size_t* out_len, uint64_t* header_rev, int* more);
/* n Lists in one call (range.go:124-174 per query), one mutex hold.
 * qbuf = n x {u32 slen; u32 elen; u64 rev; i64 limit; start; end} — the blob
 * kb_bench_range takes. rev == 0 means latest, limit <= 0 unbounded.
 * out = u32 n; n x {i32 status; i32 more; u64 header_rev; u64 len}; then the n
 * sections in query order. For status KB_OK the len section bytes are EXACTLY
 * what kb_list would have written for that query alone (u32 count; count x
 * {u64 rev; u32 klen; key; u32 vlen; val}) and `more` is kb_list's. For any
 * other status len = 0 and the status is kb_list's for that query
 * (KB_EINVALID, KB_EBADKEY, KB_EKEYTOOLONG, KB_ECOMPACTED): one bad query
 * never fails the call. header_rev is the committed revision at the call,
 * the same in every entry; rev == 0 resolves to it.
 * flags bit 0 = keys_only: every record carries vlen = 0 and no value bytes
 * (kb_bench_range mode bit 2 semantics). Any other bit: KB_EINVALID.
 * KB_ENOBUF: *out_len = required size of the whole reply, nothing is written,
 * and the same call with a larger buffer returns the same bytes.
 * n == 0 is valid (out = u32 0); n above KB_MAX_Q is served in sub-batches
 * inside the call. *total_kvs = sum of the sections' counts.
 * Sections are serialized by HIP kernels straight from the scan's winner rows
 * (DESIGN.md §3.6); a query whose answer the winner table (KB_MAX_CAP rows)
 * or the arena cannot hold whole is served by kb_list's own path with
 * identical bytes. May be interleaved freely with every other call; a
 * pending pipelined kb_bench_step batch is collected first. The call reuses
 * the gather arena, so kb_test_last_range reports an EMPTY batch (u32 0)
 * after a kb_list_batch until the next kb_bench_range / kb_bench_step. */
int kb_list_batch(kb_store*, const uint8_t* qbuf, size_t n, int flags,
                  uint8_t* out, size_t cap, size_t* out_len,
                  unsigned long long* total_kvs);
/* TEST-ONLY: the pure host reply planner of kb_list_batch (no GPU, no
 * store). Per query: status; host_len (>= 4 = size of a host-serialized
 * section, < 0 = device path whose section is 4 + dev_bytes); group (may be
 * NULL) = scan sub-batch of a device query; arena_bytes bounds the reply span
 * of one emit round (whole queries, one group). Outputs (caller arrays, may be
 * NULL): per query the directory len, the reply offset of its section and its
 * emit round (-1 = none); round_span = {lo, hi} reply offsets per round (room
 * for n pairs); *n_rounds; *required = reply size = 4 + 24 n + sum of lens.
 * Returns KB_OK, KB_ENOBUF (required > cap) or KB_EINVALID (an OK host
 * section under 4 bytes, or a device section larger than the arena). */
int kb_test_list_plan(const int* status, const long long* host_len,
                      const unsigned long long* dev_bytes, const int* group,
                      size_t n, size_t cap, unsigned long long arena_bytes,
                      unsigned long long* dir_len, unsigned long long* sec_off,
                      int* round, unsigned long long* round_span,
                      size_t* n_rounds, size_t* required);
/* n Gets in one call (range.go:34-121 per query), one mutex hold.
 * qbuf = n x {u32 klen; u64 rev; key} — the blob kb_bench_del takes, with the
 * read revision in place of prev_rev. rev == 0 means latest, as in kb_get.
 * out = u32 n; n x {i32 status; i32 has_kv; u64 header_rev; u64 mod_rev;
 * u64 vlen}; then the value bytes of every has_kv entry, back to back in
 * query order, unpadded; vlen = the number of value bytes of that entry.
 * status, has_kv, header_rev, mod_rev and the value of an entry are EXACTLY
 * what kb_get(key, rev) would have returned at that moment: not found or a
 * tombstone winner gives has_kv 0, mod_rev 0, vlen 0; header_rev =
 * max(committed revision at the call, mod_rev). Like kb_get the call
 * validates nothing about a key: one with bytes <= 0x24, an empty one or one
 * longer than 4096 B is searched for as it is. A key may repeat in a batch.
 * flags bit 0 = no_values: every entry has vlen = 0 and no bytes follow;
 * has_kv and mod_rev stay real. Any other bit: KB_EINVALID.
 * KB_ENOBUF: *out_len = required size of the whole reply, nothing is written,
 * and the same call with a larger buffer returns the same bytes.
 * n == 0 is valid (out = u32 0); n above KB_MAX_Q is served in sub-batches
 * inside the call. *total_found = number of has_kv entries.
 * The directory and the packed values are written by HIP kernels (DESIGN.md
 * §3.7); a single value larger than the arena (KB_ARENA_BYTES) is copied from
 * the value heap by the host with identical bytes. May be interleaved freely
 * with every other call; a pending pipelined kb_bench_step batch is collected
 * first. The call reuses the gather arena, so kb_test_last_range reports an
 * EMPTY batch (u32 0) after a kb_get_batch with n > 0 until the next
 * kb_bench_range / kb_bench_step. */
int kb_get_batch(kb_store*, const uint8_t* qbuf, size_t n, int flags,
                 uint8_t* out, size_t cap, size_t* out_len,
                 unsigned long long* total_found);
/* TEST-ONLY: the pure host reply planner of kb_get_batch (no GPU, no store).
 * Per query has_kv and vlen (0 without has_kv); queries i / max_q form one
 * sub-batch; arena_bytes bounds the value bytes of one emit round. Outputs
 * (caller arrays, may be NULL): per query the reply offset of its value
 * bytes and its emit round (-1 = no bytes, -2 = host path: one value larger
 * than the arena); round_span = {lo, hi} query index range per round (room
 * for n pairs; a round never spans two sub-batches or a host-path query);
 * *n_rounds; *n_host; *required = reply size = 4 + 32 n + sum of vlen;
 * *total_found = has_kv entries. Returns KB_OK, KB_ENOBUF (required > cap)
 * or KB_EINVALID (max_q == 0, or vlen != 0 without has_kv). */
int kb_test_get_plan(const int* has_kv, const unsigned long long* vlen,
                     size_t n, size_t max_q, size_t cap,
                     unsigned long long arena_bytes,
                     unsigned long long* val_off, int* round,
                     unsigned long long* round_span, size_t* n_rounds,
                     size_t* n_host, size_t* required,
                     unsigned long long* total_found);
/* backend.Count (range.go:177-205) */
int kb_count(kb_store*, const uint8_t* start, size_t slen, const uint8_t* end,
             size_t elen, uint64_t* header_rev, uint64_t* count);
/* n Counts in one call (range.go:177-205 per query), one mutex hold.
 * qbuf = the blob kb_list_batch / kb_bench_range take: n x {u32 slen; u32
 * elen; u64 rev; i64 limit; start; end}. limit is ignored: a count is the
 * total in range whatever the limit is. rev == 0 means latest.
 * out = u32 n; n x {i32 status; i32 0; u64 header_rev; u64 count} = 4 + 24 n
 * bytes. header_rev is the committed revision at the call, the same in every
 * entry. For rev == 0, status and count are EXACTLY what kb_count(start,
 * end) returns at that moment: its validation of both bounds (KB_EBADKEY,
 * KB_EKEYTOOLONG) and its compaction check, not kb_list's extra checks —
 * start >= end or an empty end is KB_OK with whatever kb_count counts
 * (normally 0). For rev != 0 (an extension: the reference's Count ignores
 * RangeRequest.Revision, etcd3 honours it) validation is the same, the
 * compaction check is made against rev (KB_ECOMPACTED as kb_list gives it)
 * and count is the number of kvs an unbounded kb_list(start, end, rev)
 * returns. A non-OK entry has count 0 and never fails the call. With
 * enable_etcd_compatibility == 0 every entry is KB_OK with count 0 and no
 * kernel runs (range.go:188-193).
 * flags must be 0, else KB_EINVALID. KB_ENOBUF (cap < 4 + 24 n): *out_len =
 * required size, nothing is written. n == 0 is valid (out = u32 0); n above
 * KB_MAX_Q is served in sub-batches inside the call. *total_count = sum of
 * the counts.
 * Every range is cut into tiles of KB_COUNT_TILE rows (a multiple of 64, at
 * least 64, default 4096) that HIP kernels count across the whole chip
 * (DESIGN.md §3.8). May be interleaved freely with every other call; a
 * pending pipelined kb_bench_step batch is collected first. The call writes
 * neither the winner tables nor the gather arena: kb_test_last_range returns
 * after it exactly the bytes it returned before it. */
int kb_count_batch(kb_store*, const uint8_t* qbuf, size_t n, int flags,
                   uint8_t* out, size_t cap, size_t* out_len,
                   unsigned long long* total_count);
/* TEST-ONLY: the pure tile map of kb_count_batch (no GPU, no store).
 * bounds = nq x {lo, hi, dlo, dhi}: per query the row range of the base run
 * and of the delta run, i.e. 2 nq segments; inverted bounds (lo > hi) hold no
 * row. tile = rows per tile (a multiple of 64, at least 64, else
 * KB_EINVALID). Outputs (caller arrays, may be NULL): pfx[2 nq + 1] = the
 * exclusive prefix of the segments' tile counts; per tile id its query, run
 * (0 base, 1 delta) and rows [r0, r1) (room for tile_cap tiles); *n_tiles.
 * Returns KB_OK, or KB_ENOBUF (*n_tiles > tile_cap: only pfx and *n_tiles
 * are written). */
int kb_test_count_plan(const long long* bounds, size_t nq, long long tile,
                       unsigned long long* pfx, int* t_query, int* t_run,
                       long long* t_r0, long long* t_r1, size_t tile_cap,
                       size_t* n_tiles);

/* ---- compaction (compact.go:31-127 + scanner.go:444-491,566-591) ---- */
int kb_compact(kb_store*, uint64_t rev, uint64_t* out_rev);

/* ---- watch (watch.go:37-159, ring.go, watcherhub.go) ---- */
long long kb_watch(kb_store*, const uint8_t* prefix, size_t plen, uint64_t rev,
                   int* status);
/* out = packed events {u32 n; n × {i32 type; u64 rev; u64 kv_rev; u32 klen;
 * key; u32 vlen; val}}. Returns KB_EWATCH_DROPPED once a slow consumer was
 * dropped (watcherhub.go:84-94: per-watcher buffer 10000). On KB_ENOBUF the
 * queue is left INTACT (*out_len = required size): retry with a larger
 * buffer and no event is lost. */
int kb_watch_poll(kb_store*, long long wid, uint8_t* out, size_t cap, size_t* out_len);
/* Poll n watchers in one call (watch.go:119-159 per watcher; watcherhub.go:78-100).
 * out = u32 n; then n x { i32 status; u32 len; len bytes }, in the order of wids[].
 * For status KB_OK the len bytes are EXACTLY what kb_watch_poll(wid) would have
 * written (u32 count; count x event). For any other status len = 0.
 * KB_ENOBUF: *out_len = required size of the whole reply, NO queue is drained,
 * and the call can be repeated with a larger buffer with the same result.
 * Nothing is written when cap < 4.
 * Per-watcher status is what kb_watch_poll returns: an unknown, cancelled or
 * slow-consumer wid gives KB_EWATCH_DROPPED (and is erased once the call
 * succeeds). A duplicate wid in wids[] returns KB_EINVALID and changes
 * nothing. n == 0 is valid (out = u32 0). *total_events = sum of the
 * per-watcher counts. May be interleaved freely with kb_watch_poll.
 * The first call arms a device payload ring (KB_WATCH_PAYLOAD_BYTES, default
 * 256 MiB, 0 = off): from then on each event is serialized once into HBM and
 * sections are assembled by HIP kernels; watchers whose
 * events are not resident there are served by the host serializer with
 * identical bytes. */
int kb_watch_poll_batch(kb_store*, const long long* wids, size_t n,
                        uint8_t* out, size_t cap, size_t* out_len,
                        unsigned long long* total_events);
void kb_watch_cancel(kb_store*, long long wid);

/* ---- streaming full-range reads (backend.ListByStream range.go:247-256 +
 * scanner.RangeStream scanner.go:129-145; batches of 300, receiver.go:118-150)
 * and GetPartitions (range.go:208-245; single partition like badger.go:52-54,
 * sharding lives above this ABI). Stream results are pinned at read_rev; a
 * compaction past read_rev mid-stream returns KB_ECOMPACTED (the reference
 * holds an engine snapshot instead). ---- */
long long kb_stream_open(kb_store*, const uint8_t* start, size_t slen,
                         const uint8_t* end, size_t elen, uint64_t rev,
                         uint64_t* read_rev, int* status);
/* out = packed kvs like kb_list; an EMPTY batch is the end marker */
int kb_stream_next(kb_store*, long long sid, uint8_t* out, size_t cap,
                   size_t* out_len);
void kb_stream_close(kb_store*, long long sid);
int kb_partitions(kb_store*, const uint8_t* start, size_t slen,
                  const uint8_t* end, size_t elen, uint8_t* out, size_t cap,
                  size_t* out_len, uint64_t* header_rev);

/* ---- cross-shard exchange (RCCL over xGMI) ----
 * The key slab shards by namespace hash across the GPUs of one node, one
 * store per GPU. A Range that spans shards mirrors the reference's
 * multi-partition fork/merge (pkg/backend/scanner/scanner.go:269-300): each
 * shard scans locally, ONE collective exchanges the sorted winner runs
 * (allgather of counts, then payload padded to the max — NCCL/RCCL has no
 * allgatherv), and every rank k-way-merges with the global limit+1 cut.
 * The ncclUniqueId travels out-of-band on the caller's bootstrap channel
 * (cgo host RPC, torch.distributed gloo, ...). */
/* rank 0 generates the 128-byte ncclUniqueId */
int kb_comm_id(uint8_t* out, size_t cap, size_t* len);
/* collective: all ranks call with the same id; one store per GPU */
int kb_comm_init(kb_store*, const uint8_t* id, size_t id_len, int rank, int world);
int kb_comm_rank(kb_store*, int* rank, int* world);
void kb_comm_free(kb_store*);
/* cross-shard Range: COLLECTIVE (all ranks, same arguments); out = the
 * kb_list wire format with the globally merged result; degrades to the
 * local List when no communicator is initialized */
int kb_range_global(kb_store*, const uint8_t* start, size_t slen,
                    const uint8_t* end, size_t elen, uint64_t rev,
                    int64_t limit, uint8_t* out, size_t cap, size_t* out_len,
                    uint64_t* header_rev, int* more);
/* TEST-ONLY: the k-way merge + global limit cut on caller-supplied packed
 * runs (no GPU, no communicator) — lets CPU tests pin the exchange's merge
 * semantics; runs_cat = world runs back to back, lens their byte lengths */
int kb_test_merge_runs(const uint8_t* runs_cat, const unsigned long long* lens,
                       int world, long long limit, uint8_t* out, size_t cap,
                       size_t* out_len, int* more);
/* TEST-ONLY: the pure host reply planner of kb_watch_poll_batch (no GPU, no
 * store). Inputs: nrefs device refs in watcher order as parallel arrays
 * {bytes, count, watcher_index}; per watcher its status and host_len (size of
 * a host-serialized section, >= 4; < 0 = device path, section = 4 + its refs'
 * bytes); cap. Outputs (caller arrays, may be NULL): per watcher the
 * directory len, the device event count and the offset of its section
 * bytes; per ref the offset of its first record; *required = reply size.
 * Returns KB_OK, KB_ENOBUF (required > cap) or KB_EINVALID (refs out of
 * order or naming a watcher that is not on the device path). */
int kb_test_wpoll_plan(const unsigned long long* ref_bytes,
                       const unsigned int* ref_count, const int* ref_widx,
                       size_t nrefs, const int* status,
                       const long long* host_len, size_t n, size_t cap,
                       unsigned int* dir_len, unsigned int* dir_count,
                       unsigned long long* sec_off,
                       unsigned long long* ref_off, size_t* required);

/* ---- revision (tso/tso.go:41-76) ---- */
unsigned long long kb_current_rev(kb_store*);
void kb_set_current_rev(kb_store*, unsigned long long rev); /* leader TSO init */

/* backend.Config.SkippedPrefixes (compact.go:108-127): comma-separated */
int kb_set_skipped_prefixes(kb_store*, const char* csv);
/* the encoded compact borders (golden-pinned by compact_test.go:36-79) */
int kb_compact_borders(kb_store*, uint8_t* out, size_t cap, size_t* out_len);

/* ---- test/ops hooks ---- */
void kb_clock_advance(kb_store*, long long seconds); /* TTL clock (scanner.go:147-177) */
int kb_flush(kb_store*); /* memtable -> HBM slab merge (normally automatic) */
/* full store dump (memtable flushed): {u32 n; n × {u32 klen; ikey; u32 vlen; val}}
 * sorted by internal key — byte-diffable against the oracle's okb_dump */
int kb_dump(kb_store*, uint8_t* out, size_t cap, size_t* out_len, uint64_t* n_rows);
int kb_event_log(kb_store*, uint8_t* out, size_t cap, size_t* out_len);

/* ---- bench support (the measured hot path; used by bench.py) ---- */
/* n Range queries in one device batch; returns total winners. mode bits:
 * 1 = d2h — results copied to pinned host memory, PIPELINED (the payload
 *     copy overlaps the next batch's kernels; call kb_sync before reading
 *     wall-clock);
 * 2 = keys_only — etcd3 RangeRequest.KeysOnly semantics: key + mod-revision
 *     per winner, no value bytes (an extension: the reference's etcd shim
 *     ignores the flag, server/etcd/kv.go:48-67).
 * mode 0 leaves results in the device arena (the `value` mode). */
int kb_bench_range(kb_store*, const uint8_t* qbuf, size_t nq, int mode,
                   unsigned long long* total_kvs, double* secs);
/* wait for in-flight pipelined D2H copies */
int kb_sync(kb_store*);
/* test hook: records of the most recent Range batch (kb_bench_range /
 * kb_bench_step; for nq > 1024 the last 1024-query sub-batch). Collects a
 * pending pipelined batch and drains in-flight D2H first. Launches no kernel.
 * src 0 = per-query device arena (plain D2H of each query's region);
 * src 1 = the pinned host buffer that batch's pipelined D2H filled
 *         (error if the batch ran without mode bit 1).
 * out: u32 nq; nq x {i64 written; i64 total; i64 bytes; i32 overflow; i32 0};
 *      then, in query order, `bytes` record bytes of each non-overflowed
 *      query (u64 rev | u32 klen | u32 vlen | key pad16 | value pad16).
 * KB_ENOBUF with *out_len = needed size when cap is too small. */
int kb_test_last_range(kb_store*, int src, uint8_t* out, size_t cap, size_t* out_len);
/* batched conditional updates (txn.go:249-265); tbuf = n × {u32 klen;
 * u64 prev_rev; u32 vlen; key; val}; out_revs[i] = new revision or 0 on CAS
 * failure */
int kb_bench_txn(kb_store*, const uint8_t* tbuf, size_t n, uint64_t* out_revs);
/* one bench step: Range batch launched async + txn batch overlapped on the
 * host while the kernels are in flight (results unchanged: kernels snapshot
 * device state at launch; writes stage host-side until the next sync).
 * mode bits as kb_bench_range, plus:
 * 4 = pipelined (excludes bit 1) — this step's Range batch stays in flight;
 *     `total` reports the PREVIOUS step's winners (first call reports 0) and
 *     kb_sync collects the final batch. Exact under MVCC: every Range reads
 *     at its fixed read_rev, so deferring collection by one step never
 *     changes results; txn CAS results (out_revs) are still returned
 *     in-step. */
int kb_bench_step(kb_store*, const uint8_t* qbuf, size_t nq,
                  const uint8_t* tbuf, size_t ntx, int mode, uint64_t* out_revs,
                  unsigned long long* total, double* secs);
/* batched deletes: dbuf = n × {u32 klen; u64 prev_rev; key} */
int kb_bench_del(kb_store*, const uint8_t* dbuf, size_t n, uint64_t* out_revs);
/* fast bulk insert == n serial Creates of fresh keys (see okb_bulk_create) */
int kb_bulk_create(kb_store*, const uint8_t* keys, const uint32_t* klens,
                   const uint8_t* vals, const uint32_t* vlens, size_t n);
/* perf counters as a JSON object (kernel-time totals from HIP events on the
 * store's stream, launch counts, rows scanned, bytes gathered) */
int kb_perf_json(kb_store*, char* out, size_t cap);
void kb_perf_reset(kb_store*);

#ifdef __cplusplus
}
#endif
#endif /* KB_SLAB_H */
