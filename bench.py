#!/usr/bin/env python3
"""bench.py — the measured hot path (BASELINE.json's 10M-key headline config
at N=1: the metric is quoted on a "10M-key MVCC slab").

Workload: 10M Pod-style keys / 1M extra live revisions (zipf 1.1) / 2%
tombstones on one MI355X; one step = 1000 ops = 900 batched Range(limit=500)
over random namespace prefixes + 100 Txn conditional updates (90/10 mix,
docs/benchmark.md-style 512B values, 300-client-style batching). `value` is
whole-job ops/s with the slab resident in HBM and Range results landing in
the device output arena; the PCIe-inclusive rates are reported separately as
`ops_per_sec_with_d2h` (full records, pipelined payload copy) and
`ops_per_sec_with_d2h_keys_only` (etcd3 KeysOnly semantics — key+mod-rev
only; the reference's shim ignores that flag, so this is an extension and is
never `value`).

A plain run (`--gpus 1 --steps N --warmup W`) does only what `value` needs:
load the keyspace, warm up, time the N steps, print the result line. `--full`
adds every other leg after the timed steps, as before: the PCIe-inclusive
rates, the configs[2] compaction sweep, the 10k-watcher fan-out leg
(configs[4] shape at N=1), the cross-shard Range leg at N>1, the host probe
and the CPU baselines. `--dump-outputs DIR` writes what the last timed step
computed as DIR/<name>.npy (see dump_outputs). The step sequence is a pure
function of the arguments, so two builds can be compared output for output.

Multi-GPU (--gpus N via torch.distributed.run): keys shard by namespace hash,
one store per GPU; the query stream routes by namespace; weak scaling
(per-GPU keyspace fixed as N grows). cpu_baseline: the oracle (kind "port")
on the host cores, bounded sample, rank 0 / N=1 only.
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np

SEED = 0x6B62
VAL_LEN = 512
LIMIT = 500
OPS_PER_STEP = 1000
RANGE_SHARE = 0.9
MAX_PRE_STEPS = 256


def log(rank, *a):
    if rank == 0:
        print(*a, file=sys.stderr, flush=True)


def make_keys(nns, per_ns):
    namespaces = [b"/registry/pods/ns-%04d" % i for i in range(nns)]
    pods = [b"/pod-%06d" % j for j in range(per_ns)]
    keys = [ns + pod for ns in namespaces for pod in pods]
    return namespaces, keys


def build_store(store, namespaces, keys, rng, extra_revs, tomb_frac, my_ns=None):
    """Load the synthetic keyspace through the normal write path. Returns the
    loaded keys and, per key index, its latest revision (uint64; 0 once the
    key is tombstoned)."""
    from concurrent.futures import ThreadPoolExecutor

    t_phase = time.time()

    def phase(name):
        nonlocal t_phase
        print(f"[load] {name}: {time.time()-t_phase:.1f}s", file=sys.stderr, flush=True)
        t_phase = time.time()

    if my_ns is not None:
        sel = [k for k in keys if k.rsplit(b"/", 1)[0] in my_ns]
    else:
        sel = keys
    n = len(sel)
    # chunked load (1M keys per call) bounds host memory at 10M-key scale
    f = store._f("bulk_create")
    CH = 1 << 20

    def gen_chunk(c0):
        ck = sel[c0:c0 + CH]
        m = len(ck)
        # full-range uint32 draws give the same byte stream (and leave the
        # generator in the same state) as one uint8 draw per byte, faster
        vals = rng.integers(0, 1 << 32, size=m * VAL_LEN // 4, dtype=np.uint32)
        klens = np.fromiter(map(len, ck), dtype=np.uint32, count=m)
        vlens = np.full(m, VAL_LEN, dtype=np.uint32)
        return m, b"".join(ck), klens, vals, vlens

    base = store.current_rev()
    # the next chunk is generated while the store ingests the current one;
    # only the worker draws from rng here, so the stream order is unchanged
    with ThreadPoolExecutor(max_workers=1) as pool:
        nxt = pool.submit(gen_chunk, 0) if n else None
        for c0 in range(0, n, CH):
            m, kblob, klens, vals, vlens = nxt.result()
            nxt = pool.submit(gen_chunk, c0 + CH) if c0 + CH < n else None
            rc = f(ctypes.c_void_p(store.h), kblob,
                   ctypes.c_void_p(klens.ctypes.data),
                   ctypes.c_void_p(vals.ctypes.data),
                   ctypes.c_void_p(vlens.ctypes.data), ctypes.c_size_t(m))
            assert rc == 0, "bulk_create failed"
    phase("bulk_create")
    # latest rev per key index tracked client-side: creates take consecutive
    # revisions in load order
    assert store.current_rev() == base + n, "bulk_create revision drift"
    revs = np.arange(base + 1, base + n + 1, dtype=np.uint64)
    # extra revisions, zipf(1.1) — batched through the C txn path
    if extra_revs and n:
        zs = ((rng.zipf(1.1, size=extra_revs) - 1) % n).tolist()
        vbuf = rng.integers(0, 256, size=VAL_LEN, dtype=np.uint8).tobytes()
        done = 0
        batch = 8192
        while done < extra_revs:
            # unique keys per batch (revs must chain between batches)
            uniq, seen = [], set()
            while done < extra_revs and len(uniq) < batch:
                ki = zs[done]
                if ki not in seen:
                    seen.add(ki)
                    uniq.append(ki)
                done += 1
            txn_batch(store, sel, uniq, revs, vbuf, must_succeed=True)
        phase("extra revisions")
    # tombstones
    if tomb_frac and n:
        nt = int(n * tomb_frac)
        idx = rng.choice(n, size=nt, replace=False)
        fdel = store._f("bench_del")
        batch = 8192
        for b0 in range(0, nt, batch):
            ki = idx[b0:b0 + batch]
            parts = []
            for i, pr in zip(ki.tolist(), revs[ki].tolist()):
                k = sel[i]
                parts.append(struct.pack("<IQ", len(k), pr))
                parts.append(k)
            out = np.empty(len(ki), dtype=np.uint64)
            rc = fdel(ctypes.c_void_p(store.h), b"".join(parts),
                      ctypes.c_size_t(len(ki)),
                      out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
            assert rc == 0
            assert out.all()
            revs[ki] = 0
        phase("tombstones")
    store._f("flush")(ctypes.c_void_p(store.h))
    phase("final fold")
    return sel, revs


def pack_queries(qs):
    parts = []
    for s, e, rev, limit in qs:
        parts.append(struct.pack("<IIQQ", len(s), len(e), rev, limit))
        parts.append(s)
        parts.append(e)
    return b"".join(parts)


def gen_step_queries(rng, namespaces, cur_rev, n):
    out = []
    for _ in range(n):
        ns = namespaces[int(rng.integers(len(namespaces)))]
        off = int(min(rng.zipf(1.1), 500))
        rev = max(1, cur_rev - off)
        out.append((ns + b"/", ns + b"0", rev, LIMIT))
    return out


def txn_batch(store, keys, idx, revs, val, must_succeed=False):
    """One conditional update of `val` per key index in idx (unique), each
    against its tracked revision; updates revs in place."""
    ia = np.asarray(idx, dtype=np.int64)
    parts = []
    for i, pr in zip(ia.tolist(), revs[ia].tolist()):
        k = keys[i]
        parts.append(struct.pack("<IQI", len(k), pr, len(val)))
        parts.append(k)
        parts.append(val)
    blob = b"".join(parts)
    out = np.empty(len(ia), dtype=np.uint64)
    rc = store._f("bench_txn")(ctypes.c_void_p(store.h), blob,
                               ctypes.c_size_t(len(ia)),
                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    assert rc == 0
    ok = out != 0
    if must_succeed and not ok.all():
        raise AssertionError(
            f"seed update failed for {keys[int(ia[~ok][0])]!r}")
    revs[ia[ok]] = out[ok]


def bench_range_call(store, blob, nq, d2h):
    f = store._f("bench_range")
    total = ctypes.c_ulonglong()
    secs = ctypes.c_double()
    rc = f(ctypes.c_void_p(store.h), blob, ctypes.c_size_t(nq),
           ctypes.c_int(1 if d2h else 0), ctypes.byref(total), ctypes.byref(secs))
    assert rc == 0
    return total.value, secs.value


def _load_full_cpu_baseline():
    try:
        d = json.load(open(os.path.join(REPO, "profiles",
                                        "cpu_full_baseline.json")))
        return {"value": d["value"], "unit": d["unit"], "cores": d["cores"],
                "kind": d["kind"], "note": d["what"]}
    except Exception:
        return None


def perf(store):
    buf = ctypes.create_string_buffer(4096)
    rc = store._f("perf_json")(ctypes.c_void_p(store.h), buf, ctypes.c_size_t(4096))
    assert rc == 0
    return json.loads(buf.value.decode())


def run_txns(store, keys, live, revs, rng, n):
    vbuf = rng.integers(0, 256, size=VAL_LEN, dtype=np.uint8).tobytes()
    idx, seen = [], set()
    while len(idx) < n:
        ki = int(live[int(rng.integers(len(live)))])
        if revs[ki] == 0 or ki in seen:
            continue
        seen.add(ki)
        idx.append(ki)
    txn_batch(store, keys, idx, revs, vbuf)


def cross_shard_leg_wrapper(store, dist, pg, rank, world, all_namespaces):
    # the product path: kb_comm_init + kb_range_global (RCCL over xGMI inside
    # the C-ABI, comm.cc). Falls back to the torch.distributed emulation only
    # if the C-ABI path cannot run (e.g. the CPU gloo rehearsal's mock store).
    try:
        return cross_shard_cabi(store, dist, rank, world, all_namespaces)
    except Exception as e:  # noqa: BLE001
        out = cross_shard_leg(store, dist, pg, rank, world, all_namespaces)
        out["cabi_fallback_reason"] = repr(e)[:200]
        return out


def cross_shard_cabi(store, dist, rank, world, all_namespaces, n_queries=64,
                     limit=LIMIT):
    """configs[3] through the product C-ABI: every rank scans its shard and
    kb_range_global runs the RCCL allgather(counts)+allgather(payload) over
    xGMI plus the k-way merge with the global limit cut (comm.cc; semantics
    scanner.go:269-300). The ncclUniqueId bootstraps out-of-band over the
    gloo group."""
    import ctypes as C

    import torch

    from kubebrain_amd.client import _parse_kvs

    lib = store.lib
    idb = C.create_string_buffer(256)
    idlen = C.c_size_t()
    if rank == 0:
        rc = lib.kb_comm_id(idb, C.c_size_t(256), C.byref(idlen))
        assert rc == 0, f"kb_comm_id rc={rc}"
        idt = torch.frombuffer(bytearray(idb.raw[:128]), dtype=torch.uint8).clone()
    else:
        idt = torch.zeros(128, dtype=torch.uint8)
    dist.broadcast(idt, src=0)  # gloo (CPU) bootstrap channel
    id_bytes = bytes(idt.numpy().tobytes())
    rc = lib.kb_comm_init(C.c_void_p(store.h), id_bytes, C.c_size_t(128),
                          C.c_int(rank), C.c_int(world))
    assert rc == 0, f"kb_comm_init rc={rc}"
    try:
        BUF = 8 << 20
        out = C.create_string_buffer(BUF)
        merged_counts = []
        t0 = time.time()
        for qi in range(n_queries):
            lo = b"/registry/pods/ns-%04d" % (qi % max(len(all_namespaces) // 2, 1))
            hi = b"/registry/pods0"
            out_len = C.c_size_t()
            hr = C.c_uint64()
            more = C.c_int()
            rc = lib.kb_range_global(C.c_void_p(store.h), lo, C.c_size_t(len(lo)),
                                     hi, C.c_size_t(len(hi)), C.c_uint64(0),
                                     C.c_longlong(limit), out, C.c_size_t(BUF),
                                     C.byref(out_len), C.byref(hr), C.byref(more))
            assert rc == 0, f"kb_range_global rc={rc}"
            if rank == 0:
                kvs = _parse_kvs(out.raw[:out_len.value])
                assert all(kvs[i].key < kvs[i + 1].key
                           for i in range(len(kvs) - 1)), "merge order"
                merged_counts.append(len(kvs))
        dt = time.time() - t0
    finally:
        lib.kb_comm_free(C.c_void_p(store.h))
    return {
        "queries": n_queries,
        "ops_per_sec": round(n_queries / dt, 1),
        "limit": limit,
        "transport": "rccl-cabi (kb_range_global over xGMI)",
        "merged_counts_min_max": [min(merged_counts), max(merged_counts)]
        if merged_counts else None,
    }


def cross_shard_leg(store, dist, pg, rank, world, all_namespaces, n_queries=64,
                    limit=LIMIT):
    """configs[3]: cross-shard Range — every shard scans its sub-slab, winner
    payloads are exchanged with one collective (RCCL over xGMI when CUDA is
    up, the gloo group otherwise), and rank 0 k-way-merges the sorted runs
    with the global limit+1 cut (semantics pinned by
    tests/test_gloo_shard.py)."""
    import heapq

    import torch

    use_cuda = torch.cuda.is_available()
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0))) \
        if use_cuda else torch.device("cpu")
    t0 = time.time()
    merged_counts = []
    for qi in range(n_queries):
        # a cross-namespace range spanning every shard
        lo = b"/registry/pods/ns-%04d" % (qi % max(len(all_namespaces) // 2, 1))
        r = store.list(lo, b"/registry/pods0", 0, limit + 1)
        parts = [struct.pack("<QII", kv.revision, len(kv.key), len(kv.value))
                 + kv.key + kv.value for kv in r.kvs]
        blob = b"".join(parts)
        # exchange: lengths then padded payload (allgatherv emulation)
        ln = torch.tensor([len(blob)], dtype=torch.int64, device=dev)
        lens = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(lens, ln, group=pg)
        mx = int(max(x.item() for x in lens))
        buf = torch.zeros(mx, dtype=torch.uint8, device=dev)
        if blob:
            buf[:len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
        outs = [torch.zeros(mx, dtype=torch.uint8, device=dev) for _ in range(world)]
        dist.all_gather(outs, buf, group=pg)
        if rank == 0:
            runs = []
            for rr in range(world):
                data = bytes(outs[rr][: int(lens[rr].item())].cpu().numpy().tobytes())
                run, off = [], 0
                while off < len(data):
                    rev, klen, vlen = struct.unpack_from("<QII", data, off)
                    off += 16
                    k = data[off:off + klen]; off += klen
                    v = data[off:off + vlen]; off += vlen
                    run.append((k, rev, v))
                runs.append(run)
            merged = list(heapq.merge(*runs, key=lambda kv: kv[0]))[: limit]
            assert all(merged[i][0] < merged[i + 1][0]
                       for i in range(len(merged) - 1)), "merge order"
            merged_counts.append(len(merged))
    dt = time.time() - t0
    return {
        "queries": n_queries * 1,
        "ops_per_sec": round(n_queries / dt, 1),
        "limit": limit,
        "transport": "nccl(RCCL/xGMI)" if use_cuda else "gloo",
        "merged_counts_min_max": [min(merged_counts), max(merged_counts)]
        if rank == 0 and merged_counts else None,
    }


def cpu_baseline_leg(namespaces, keys, sample_qs):
    """Oracle (CPU restatement, kind 'port') on the host cores — the only
    bench.py use of oracle/ (DESIGN.md §1)."""
    from kbclient import open_oracle

    rng = np.random.default_rng(SEED)
    o = open_oracle()
    o.set_current_rev(1000)
    t0 = time.time()
    # bounded sample: a slice of the keyspace big enough for real ranges
    ns_n = min(len(namespaces), 200)
    sub_ns = namespaces[:ns_n]
    sub_keys = [k for k in keys if k.rsplit(b"/", 1)[0] in set(sub_ns)]
    n = len(sub_keys)
    vals = rng.integers(0, 256, size=n * VAL_LEN, dtype=np.uint8).tobytes()
    klens = (ctypes.c_uint32 * n)(*[len(k) for k in sub_keys])
    vlens = (ctypes.c_uint32 * n)(*([VAL_LEN] * n))
    f = o.lib.okb_bulk_create
    rc = f(ctypes.c_void_p(o.h), b"".join(sub_keys), klens, vals, vlens,
           ctypes.c_size_t(n))
    assert rc == 0
    build_s = time.time() - t0
    threads = os.cpu_count() or 1
    # queries clamped to the loaded namespaces
    qs = []
    qrng = np.random.default_rng(SEED + 7)
    for _ in range(4000):
        ns = sub_ns[int(qrng.integers(len(sub_ns)))]
        qs.append((ns + b"/", ns + b"0", 0, LIMIT))
    blob = pack_queries(qs)
    fb = o.lib.okb_bench_range
    # bounded sample: repeat the query batch until >=5s of CPU work
    tot_q, tot_s = 0, 0.0
    while tot_s < 5.0:
        total = ctypes.c_ulonglong()
        secs = ctypes.c_double()
        rc = fb(ctypes.c_void_p(o.h), blob, ctypes.c_size_t(len(qs)),
                ctypes.c_int(threads), ctypes.byref(total), ctypes.byref(secs))
        assert rc == 0
        tot_q += len(qs)
        tot_s += secs.value
    range_ops_s = tot_q / tot_s
    secs = ctypes.c_double(tot_s)
    # txn rate (single-writer, as the reference serializes writes):
    # successful conditional updates with the tracked revision
    base = 1000
    revs = {k: base + i + 1 for i, k in enumerate(sub_keys)}
    t0 = time.time()
    ntx = 2000
    vx = b"x" * VAL_LEN
    for i in range(ntx):
        k = sub_keys[i % len(sub_keys)]
        r = o.update(k, vx, revs[k])
        assert r.succeeded
        revs[k] = r.header_revision
    txn_s = time.time() - t0
    txn_ops_s = ntx / txn_s
    o.close()
    mix = 1.0 / (RANGE_SHARE / range_ops_s + (1 - RANGE_SHARE) / txn_ops_s)
    return {
        "value": round(mix, 1),
        "unit": "ops/s",
        "cores": threads,
        "kind": "port",
        "sample": f"{ns_n} namespaces/{n} keys subset; {tot_q} Range(limit=500) "
                  f"on {threads} threads ({tot_s:.1f}s) + {ntx} serial txns "
                  f"({txn_s:.1f}s); mix = harmonic 90/10; build {build_s:.1f}s",
        "range_ops_per_sec": round(range_ops_s, 1),
        "txn_ops_per_sec": round(txn_ops_s, 1),
    }


def watch_leg(store, namespaces, keys, live, revs, rng, n_watchers, n_events):
    """configs[4]-shaped fan-out: n_watchers live watchers, n_events writes.
    `delivered` counts events landed in watcher queues (bitmap references —
    the same cost model as the reference's shared-batch-pointer fan-out,
    watcherhub.go:78-100); a 100-watcher poll sample then materializes full
    events from the ring to show the consumer-side path at rate."""
    import kbclient
    wids = []
    for i in range(n_watchers):
        if i % 5 == 0:
            pfx = b"/registry/pods/"
        else:
            pfx = namespaces[int(rng.integers(len(namespaces)))] + b"/"
        st, wid = store.watch(pfx, 0)
        assert st == kbclient.OK
        wids.append(wid)
    p0 = perf(store)
    t0 = time.time()
    run_txns(store, keys, live, revs, rng, n_events)
    # final pump via a poll
    store.watch_poll(wids[0])
    dt = time.time() - t0
    p1 = perf(store)
    delivered = p1.get("delivered", 0) - p0.get("delivered", 0)
    # poll sample: materialize events for 100 watchers (incl. heavy ones)
    t0 = time.time()
    polled = 0
    for wid in wids[:100]:
        rc, evs = store.watch_poll(wid)
        if rc == kbclient.OK:
            polled += len(evs)
    poll_dt = time.time() - t0
    stats = {
        "delivered": delivered,
        "filter_ms": round(p1.get("filter_ms", 0) - p0.get("filter_ms", 0), 3),
        "filter_launches": p1.get("filter_launches", 0) - p0.get("filter_launches", 0),
        "poll_sample": {"watchers": 100, "events": polled,
                        "events_per_sec": round(polled / poll_dt, 1) if poll_dt > 0 else None},
    }
    for wid in wids:
        store.watch_cancel(wid)
    return delivered / dt if dt > 0 else 0.0, delivered, stats


DUMP_SAMPLE_QUERIES = 8


def dump_outputs(out_dir, store, queries, step_totals, txn_revs, suffix=""):
    """Write what the last timed step computed as <out_dir>/<name>.npy.

    What kb_bench_step hands its caller:
      step_range_totals  float64 [steps]  Range rows reported by each timed
                                          call (pipelined: step k reports the
                                          batch launched by step k-1)
      txn_revisions      float64 [ntx]    new revision of each conditional
                                          update of the last step (0 = CAS
                                          failed)
    The Range records themselves stay in the device output arena, so the
    last step's query batch is read back through the List API at the same
    read revisions (snapshot-exact, so later writes do not change it):
      range_counts       float64 [nq]         rows returned per query
      range_more         float64 [nq]         the More flag per query
      range_revisions    float64 [nq, LIMIT]  mod revision per row (0 pad)
      range_crc32        float64 [nq, LIMIT]  crc32(key + value) per row
      range_sample_values float32 [8, LIMIT, VAL_LEN]  value bytes of a
                                          fixed seeded sample of 8 queries
    About 16 MB at the default shape."""
    import zlib

    os.makedirs(out_dir, exist_ok=True)
    nq = len(queries)
    counts = np.zeros(nq, dtype=np.float64)
    more = np.zeros(nq, dtype=np.float64)
    rows_rev = np.zeros((nq, LIMIT), dtype=np.float64)
    rows_crc = np.zeros((nq, LIMIT), dtype=np.float64)
    ns = min(DUMP_SAMPLE_QUERIES, nq)
    sample = sorted(np.random.default_rng(SEED).choice(nq, size=ns,
                                                       replace=False).tolist())
    values = np.zeros((ns, LIMIT, VAL_LEN), dtype=np.float32)
    for qi, (s, e, rev, limit) in enumerate(queries):
        r = store.list(s, e, rev, limit)
        assert r.status == 0, f"dump read-back failed: status {r.status}"
        counts[qi] = len(r.kvs)
        more[qi] = float(r.more)
        slot = sample.index(qi) if qi in sample else -1
        for j, kv in enumerate(r.kvs[:LIMIT]):
            rows_rev[qi, j] = kv.revision
            rows_crc[qi, j] = zlib.crc32(kv.key + kv.value)
            if slot >= 0:
                v = np.frombuffer(kv.value[:VAL_LEN], dtype=np.uint8)
                values[slot, j, :len(v)] = v
    arrays = {
        "step_range_totals": np.asarray(step_totals, dtype=np.float64),
        "txn_revisions": np.asarray(txn_revs, dtype=np.float64),
        "range_counts": counts,
        "range_more": more,
        "range_revisions": rows_rev,
        "range_crc32": rows_crc,
        "range_sample_values": values,
    }
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, name + suffix + ".npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    # the headline config (BASELINE.json metric): 10M keys / 1M extra revs
    ap.add_argument("--nns", type=int, default=2000)
    ap.add_argument("--per-ns", type=int, default=5000)
    ap.add_argument("--extra-revs", type=int, default=1000000)
    ap.add_argument("--watchers", type=int, default=10000)
    ap.add_argument("--watch-events", type=int, default=6000)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other leg "
                         "(PCIe-inclusive rates, compaction sweep, watch "
                         "fan-out, cross-shard Range at N>1, host probe, CPU "
                         "baselines) and add their keys to the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one "
                         "computed as DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--spin-up", type=float, default=2.0, metavar="SECONDS",
                    help="sustained range-only load before the warmup steps, "
                         "so the clocks reach steady boost (default 2.0)")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU baseline leg")
    ap.add_argument("--no-compact-bench", action="store_true",
                    help="with --full: skip the compaction-sweep leg "
                         "(configs[2] shape)")
    args = ap.parse_args()
    t_start = time.time()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    dist = None
    if world > 1:
        import torch
        import torch.distributed as tdist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        tdist.init_process_group(backend="gloo", rank=rank, world_size=world)
        dist = tdist
        os.environ["KB_DEVICE"] = str(local_rank)

    # weak scaling (SURVEY §8e / configs[3]): per-GPU keyspace fixed, total
    # keys grow with N (N x 1M at the defaults)
    if world > 1:
        args.nns *= world
        args.extra_revs *= world
        args.watchers *= world
        args.watch_events *= world

    # device capacity sizing for this workload
    total_rows = int((args.nns * args.per_ns * 2.1 + args.extra_revs) * 1.6 / world)
    os.environ.setdefault("KB_MAX_ROWS", str(max(total_rows, 1 << 20)))
    os.environ.setdefault("KB_HEAP_BYTES",
                          str(int((args.nns * args.per_ns / world + args.extra_revs)
                                  * (VAL_LEN + 16) * 1.4) + (128 << 20)))
    # delta-run fold threshold; syncs happen at every read batch (timed)
    os.environ.setdefault("KB_FLUSH_ROWS", "262144")
    # the unbounded host event log is for parity tests, not the bench
    os.environ.setdefault("KB_EVENT_LOG", "0")

    import kubebrain_amd

    # torch is first needed at the barrier before the timed steps; importing
    # it takes seconds, so it loads in the background while the store ingests
    # the keyspace (the load sits in native code and does not hold the GIL)
    import importlib
    import threading
    torch_import = threading.Thread(target=importlib.import_module,
                                    args=("torch",), daemon=True)
    torch_import.start()

    import zlib
    namespaces, keys = make_keys(args.nns, args.per_ns)
    # namespace-hash sharding (same routing as tests/test_gloo_shard)
    my_ns = set(ns for ns in namespaces if zlib.crc32(ns) % world == rank)

    store = kubebrain_amd.open_store(store_prefix=b"/registry")
    store.set_current_rev(1000)
    rng = np.random.default_rng(SEED + rank)
    log(rank, f"[bench] loading shard rank={rank}/{world} "
              f"({len(my_ns)} namespaces)...")
    t0 = time.time()
    sel, revs = build_store(store, namespaces, keys, rng,
                            args.extra_revs // world, 0.02,
                            my_ns if world > 1 else None)
    live = np.flatnonzero(revs)  # key indices not tombstoned
    log(rank, f"[bench] loaded {len(sel)} keys in {time.time()-t0:.1f}s; "
              f"slab={perf(store)['slab_rows']} rows")

    my_ns_list = sorted(my_ns)
    qrng = np.random.default_rng(SEED + 100 + rank)

    # pre-generate the query stream AND the txn batches (client-side work,
    # outside the measured server path — the reference bench's 300 clients
    # generate requests too). Txn batches use keys disjoint across steps, so
    # each key's prev-rev is known at generation time; returned revisions
    # update the client map after each step.
    nq = int(OPS_PER_STEP * RANGE_SHARE)  # 900 ranges
    ntx = OPS_PER_STEP - nq               # 100 txns
    # The stream is bounded, so that generating it stays a small fixed cost
    # at any --steps: longer runs cycle through the pre-generated steps.
    n_pre = min(args.warmup + args.steps + max(2, args.steps // 8) + 2,
                MAX_PRE_STEPS)
    cur = store.current_rev()
    pre_qs = [gen_step_queries(qrng, my_ns_list, cur, nq) for _ in range(n_pre)]
    pre_blobs = [pack_queries(qs) for qs in pre_qs]
    vbuf = qrng.integers(0, 256, size=VAL_LEN, dtype=np.uint8).tobytes()
    tx_idx, seen_tx = [], set()
    for _ in range(n_pre):
        ks, step_seen, attempts = [], set(), 0
        while len(ks) < ntx:
            attempts += 1
            if attempts > 20 * ntx or len(seen_tx) >= max(len(live) - ntx, 0):
                seen_tx.clear()  # small pools: reuse keys (stale prev-revs
                # then CAS-fail, which is legitimate mix noise; the default
                # 1M-key config never reuses)
            ki = int(live[int(qrng.integers(len(live)))])
            if ki in seen_tx or ki in step_seen or revs[ki] == 0:
                continue
            seen_tx.add(ki)
            step_seen.add(ki)
            ks.append(ki)
        tx_idx.append(np.array(ks, dtype=np.int64))
    tx_keys = [[sel[ki] for ki in ia.tolist()] for ia in tx_idx]
    fstep = store._f("bench_step")
    tx_out = np.empty(ntx, dtype=np.uint64)
    tx_out_ptr = tx_out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    step_i = [0]

    t_split = {"range_s": 0.0, "txn_s": 0.0}

    def one_step(mode=0, txns=True):
        # one call: range batch launched async, txn batch overlapped on the
        # host while the kernels are in flight (kb_bench_step). mode bit0 =
        # d2h (pipelined payload copy), bit1 = keys_only, bit2 = pipelined.
        # The txn blob is packed HERE, per step, from the tracked revisions:
        # pre-built blobs go stale once the key pool cycles and every CAS
        # then fails, silently dropping the write half of the 90/10 mix.
        # txns=False sends the range batch alone and leaves the store as it
        # was (the spin-up steps before warmup).
        i = step_i[0] % n_pre
        step_i[0] += 1
        ia = tx_idx[i]
        parts = []
        if txns:
            for k, pr in zip(tx_keys[i], revs[ia].tolist()):
                parts.append(struct.pack("<IQI", len(k), pr, VAL_LEN))
                parts.append(k)
                parts.append(vbuf)
        tx_blob = b"".join(parts)
        total = ctypes.c_ulonglong()
        secs = ctypes.c_double()
        rc = fstep(ctypes.c_void_p(store.h), pre_blobs[i], ctypes.c_size_t(nq),
                   tx_blob, ctypes.c_size_t(ntx if txns else 0),
                   ctypes.c_int(mode), tx_out_ptr,
                   ctypes.byref(total), ctypes.byref(secs))
        assert rc == 0
        t_split["range_s"] += secs.value
        if txns:
            ok = tx_out != 0
            revs[ia[ok]] = tx_out[ok]
        return total.value

    def drain():
        assert store._f("sync")(ctypes.c_void_p(store.h)) == 0

    torch_import.join()
    import torch

    def barrier():
        if dist:
            dist.barrier()
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    # warmup: args.warmup steps AND >= 2s (--spin-up) of sustained load, so
    # the clock governor reaches steady boost before the timed region (short
    # warmups showed ~2x run-to-run variance across hosts). The time-bound
    # part comes first and sends range batches only: how many of them fit in
    # 2s varies from run to run, and they must not move the store's
    # revisions, or the timed steps' inputs would differ from run to run.
    log(rank, f"[bench] setup done {time.time()-t_start:.1f}s after start")
    t0 = time.time()
    spin = 0
    while time.time() - t0 < args.spin_up and spin < 10000:
        one_step(mode=4, txns=False)
        spin += 1
    drain()
    step_i[0] = 0  # warmup and timed steps always use the same stream
    for _ in range(args.warmup):
        one_step(mode=4)  # pipelined: previous batch collected next step
    drain()
    barrier()
    store._f("perf_reset")(ctypes.c_void_p(store.h))
    t_split["range_s"] = t_split["txn_s"] = 0.0
    step_totals = []
    t0 = time.time()
    for _ in range(args.steps):
        step_totals.append(one_step(mode=4))
    drain()  # finish the in-flight final batch inside the timed bracket
    barrier()
    elapsed = time.time() - t0
    split_snapshot = dict(t_split)  # before the untimed d2h/watch phases
    if dist:
        import torch as _t
        e = _t.tensor([elapsed])
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e.item())
    p = perf(store)
    log(rank, f"[bench] timed {args.steps} steps in {elapsed:.3f}s")

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, store,
                     pre_qs[(step_i[0] - 1) % n_pre] if args.steps else [],
                     step_totals, tx_out.copy() if args.steps else [],
                     suffix=f"_rank{rank}" if world > 1 else "")
        log(rank, f"[bench] outputs written to {args.dump_outputs}")

    total_ops = OPS_PER_STEP * args.steps * world
    value = total_ops / elapsed
    # roofline over the range path (scan + winner gather), per SURVEY §8d's
    # algorithmic bytes: 16B per row scanned (meta+rev) +
    # gathered record bytes (key+value+header per winner)
    rng_s = (p["scan_ms"] + p["gather_ms"]) / 1e3
    alg_bytes = p["rows_scanned"] * 16 + p["bytes_gathered"]
    achieved = alg_bytes / rng_s if rng_s > 0 else 0.0
    peak = 8.0e12
    roofline = {
        "bound": "hbm",
        "achieved": round(achieved / 1e9, 2),
        "peak": peak / 1e9,
        "unit": "GB/s",
        "frac": round(achieved / peak, 4),
        "traffic": None,  # filled below from the committed PMC sidecar
        "kernel": "k_range_scan+k_gather",
        "scan_only_GBps": round((p["rows_scanned"] * 16) / (p["scan_ms"] / 1e3) / 1e9, 2)
                          if p["scan_ms"] > 0 else None,
        "note": "achieved = (rows_scanned x 16B + gathered bytes) / HIP-event "
                "kernel time on the store stream",
    }

    # PMC-measured HBM traffic per launch (profiles/pmc_traffic.json,
    # collected with rocprofv3 --pmc FETCH_SIZE on this same workload)
    try:
        tj = json.load(open(os.path.join(REPO, "profiles", "pmc_traffic.json")))
        per_launch = (tj["scan_bytes_per_launch"] * tj.get("scan_correction", 1)
                      + tj["gather_bytes_per_launch"])
        roofline["traffic"] = int(per_launch)
        roofline["traffic_note"] = tj["_source"]
    except Exception:
        pass

    # the result line of a plain run: the headline figure and what the timed
    # steps' own counters give for free (--full adds the other legs' keys)
    result = {
        "metric": "range+txn ops/s (90/10, Range limit=500) + watch events/s",
        "value": round(value, 1),
        "unit": "ops/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
        "config": {
            "workload": f"10M-key MVCC slab headline config: "
                        f"{args.nns * args.per_ns // 1000000}M Pod-style keys / "
                        f"{args.extra_revs} extra revisions (zipf 1.1) / 2% "
                        f"tombstones, Range(limit=500)+Txn conditional-update "
                        f"90/10, 512B values, single MI355X"
                        if world == 1 else
                        f"10M-key headline config sharded by namespace hash "
                        f"over {world} GPUs (weak scaling)",
            "n_keys": args.nns * args.per_ns,
            "extra_revs": args.extra_revs,
            "limit": LIMIT,
            "ops_per_step": OPS_PER_STEP,
            "watchers": max(args.watchers // world, 8) * world,
        },
        "step_split_ms": {"range": round(split_snapshot["range_s"] / args.steps * 1e3, 3),
                          "txn": round(split_snapshot["txn_s"] / args.steps * 1e3, 3)},
        "roofline": roofline,
        "perf": p,
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(result))
        if dist:
            dist.destroy_process_group()
        return

    # ---- --full only from here: every leg below takes runs of its own ----

    # one-off PCIe reference: pinned D2H bandwidth of the host (torch copy)
    # host-health probe: host spin speed + GPU sclk, reported with the line
    # (host-to-host variance reaches 3x; a slow `value` with a slow probe is
    # the machine, not the code)
    box = {}
    try:
        t0 = time.time()
        x = 0
        for i in range(3_000_000):
            x += i * i
        box["host_spin_ms"] = round((time.time() - t0) * 1e3, 1)
        import subprocess
        out = subprocess.run(["rocm-smi", "--showgpuclocks", "--csv"],
                             capture_output=True, text=True, timeout=10).stdout
        for tok in out.replace(",", " ").split():
            if tok.endswith("Mhz") or tok.endswith("MHz"):
                box["sclk_mhz"] = int("".join(c for c in tok if c.isdigit()))
                break
    except Exception:
        pass

    pcie_gbps = None
    if torch.cuda.is_available():
        try:
            src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
            dst = torch.empty(256 << 20, dtype=torch.uint8, pin_memory=True)
            dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(4):
                dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            pcie_gbps = round(4 * (256 << 20) / (time.time() - t0) / 1e9, 1)
            del src, dst
        except Exception:
            pass

    # PCIe-inclusive measurement (separate, untimed-region): full records,
    # payload copy pipelined across steps (kb_sync drains the tail before the
    # clock stops). Two untimed warmup steps first: the first pipelined call
    # allocates the ping-pong pack arenas + pinned staging (~1s one-off).
    def d2h_leg(mode, n_steps):
        for _ in range(2):
            one_step(mode=mode)
        drain()
        p0 = perf(store)
        t0 = time.time()
        for _ in range(n_steps):
            one_step(mode=mode)
        drain()
        dt = time.time() - t0
        p1 = perf(store)
        detail = {
            "wall_ms_per_step": round(dt / n_steps * 1e3, 3),
            "pack_d2h_ms_per_step": round(
                (p1["pack_d2h_ms"] - p0["pack_d2h_ms"]) / n_steps, 3),
            "kernel_ms_per_step": round(
                (p1["scan_ms"] + p1["gather_ms"] - p0["scan_ms"] - p0["gather_ms"])
                / n_steps, 3),
            "get_ms_per_step": round((p1["get_ms"] - p0["get_ms"]) / n_steps, 3),
            "MB_per_step": round((p1["bytes_gathered"] - p0["bytes_gathered"])
                                 / n_steps / 1e6, 1),
            "sync_s": round(p1["sync_s"] - p0["sync_s"], 3),
        }
        return dt, detail

    d2h_steps = max(4, args.steps // 4)
    d2h_elapsed, d2h_detail = d2h_leg(1, d2h_steps)
    # keys-only variant (etcd3 KeysOnly semantics; response payload is
    # key + mod-revision per winner — an extension, see module docstring)
    d2h_ko_elapsed, d2h_ko_detail = d2h_leg(3, d2h_steps)

    # cross-shard Range leg (configs[3]) at N>1: RCCL/xGMI exchange + merge.
    # Exception-guarded: a failure degrades to a JSON note, never the run.
    cross_shard = None
    if world > 1:
        try:
            pg = None
            import torch as _t
            if _t.cuda.is_available():
                pg = dist.new_group(backend="nccl")
            cross_shard = cross_shard_leg_wrapper(store, dist, pg, rank, world,
                                                  namespaces)
        except Exception as e:  # noqa: BLE001
            cross_shard = {"error": repr(e)[:300]}

    # compaction sweep leg (configs[2]: drop revisions < compactRev; the
    # sweep reads the whole slab and stream-compacts rows + value heap)
    compact_stats = None
    if not args.no_compact_bench:
        p_pre = perf(store)
        rows_pre = p_pre["slab_rows"]
        heap_pre = p_pre["heap_used"]
        t0 = time.time()
        rc, crev = store.compact(0)
        csecs = time.time() - t0
        assert rc == 0
        p_post = perf(store)
        sweep_bytes = rows_pre * 112 + p_post["slab_rows"] * 112 \
            + heap_pre + p_post["heap_used"]
        compact_stats = {
            "seconds": round(csecs, 4),
            "rows_before": rows_pre,
            "rows_after": p_post["slab_rows"],
            "heap_before": heap_pre,
            "heap_after": p_post["heap_used"],
            "device_ms": round(p_post["compact_ms"] - p_pre["compact_ms"], 3),
            "algorithmic_GBps": round(sweep_bytes / max(
                (p_post["compact_ms"] - p_pre["compact_ms"]) / 1e3, 1e-9) / 1e9, 2),
            "compact_rev": crev,
        }
        log(rank, f"[bench] compact sweep: {compact_stats}")

    # watch fan-out leg
    wrate, delivered, watch_stats = watch_leg(store, my_ns_list, sel, live,
                                              revs, qrng,
                                              max(args.watchers // world, 8),
                                              args.watch_events // world)
    if dist:
        import torch as _t
        w = _t.tensor([wrate])
        dist.all_reduce(w, op=dist.ReduceOp.SUM)
        wrate = float(w.item())

    cpu_baseline = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        log(rank, "[bench] cpu baseline (oracle, bounded sample)...")
        cpu_baseline = cpu_baseline_leg(namespaces, keys, [])

    if rank == 0:
        result.update({
            "cross_shard_range": cross_shard,
            "compact_sweep": compact_stats,
            "watch_events_per_sec": round(wrate, 1),
            "watch_delivered_rank0": delivered,
            "watch_stats": watch_stats,
            "ops_per_sec_with_d2h": round(OPS_PER_STEP * d2h_steps * world / d2h_elapsed, 1),
            "ops_per_sec_with_d2h_keys_only": round(
                OPS_PER_STEP * d2h_steps * world / d2h_ko_elapsed, 1),
            "d2h_detail": d2h_detail,
            "d2h_keys_only_detail": d2h_ko_detail,
            "pcie_d2h_GBps": pcie_gbps,
            "box": box,
            "cpu_baseline": cpu_baseline,
            # one-off FULL-keyspace CPU measurement (tests/cpu_full_baseline.py
            # on a 256-core host; committed artifact — the in-run bounded
            # sample above overstates the CPU, its subset being
            # cache-friendlier)
            "cpu_baseline_full_config": _load_full_cpu_baseline(),
        })
        print(json.dumps(result))
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
