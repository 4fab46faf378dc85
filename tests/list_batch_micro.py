"""GPU micro-benchmark of the public Range path (not a pytest): Q queries
served by a loop of Q kb_list calls (one query per call: gather arena, pack,
D2H, host parse, second serialization) versus ONE kb_list_batch (sections
serialized on the device from the scan's winner rows), full
values and keys_only.

One process, one store, K keys in bench-shaped namespaces
(/registry/pods/ns-XXXX/pod-XXXXX) with V-byte values, Q namespace queries of
limit L. Rounds alternate between the paths so drift hits all alike; all are
warmed first. Only the C calls are timed; nothing is parsed into Python
objects inside the timed region. kb_list has no keys_only mode, so the
keys_only batch is set against the same loop. Per path it reports wall time,
kvs/s and reply bytes/s with the round-to-round spread; for the batch also the
kernel, scan and D2H time and the bytes moved (kb_perf_json list_* counters).

The measuring step runs in a child process under its own time limit:

    python tests/list_batch_micro.py --out profiles/list_batch.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COUNTERS = ("list_ms", "list_d2h_ms", "scan_ms", "list_batch_bytes",
            "list_batch_q_dev", "list_batch_q_host", "list_batch_kvs",
            "list_emit_launches", "gather_launches")


def perf(store):
    buf = C.create_string_buffer(8192)
    store._f("perf_json")(C.c_void_p(store.h), buf, C.c_size_t(8192))
    return json.loads(buf.value.decode())


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3),
            "max": round(max(xs), 3)}


def worker(args):
    os.environ.setdefault("KB_MAX_ROWS", str(4 << 20))
    os.environ.setdefault("KB_HEAP_BYTES", str(1 << 30))
    os.environ.setdefault("KB_FLUSH_ROWS", "262144")
    os.environ.setdefault("KB_EVENT_LOG", "0")
    import kubebrain_amd
    from kubebrain_amd.client import ENOBUF, OK

    s = kubebrain_amd.open_store()
    s.set_current_rev(1000)
    h = C.c_void_p(s.h)
    per_ns = args.keys // args.namespaces
    nss = [b"/registry/pods/ns-%04d" % i for i in range(args.namespaces)]
    blob = np.random.default_rng(7).integers(0x30, 0x7b, size=1 << 20,
                                             dtype=np.uint8).tobytes()
    bulk = s._f("bulk_create")
    for ns in nss:                       # one kb_bulk_create per namespace
        keys = [ns + b"/pod-%05d" % j for j in range(per_ns)]
        klens = (C.c_uint32 * per_ns)(*[len(k) for k in keys])
        vlens = (C.c_uint32 * per_ns)(*([args.value_bytes] * per_ns))
        o = (len(ns) * 131) % 4096
        vals = b"".join(blob[o + 37 * j:o + 37 * j + args.value_bytes]
                        for j in range(per_ns))
        rc = bulk(h, b"".join(keys), klens, vals, vlens, C.c_size_t(per_ns))
        assert rc == 0, rc
    qs = [(nss[(i * 7) % len(nss)] + b"/", nss[(i * 7) % len(nss)] + b"0", 0,
           args.limit) for i in range(args.queries)]
    qbuf = s.encode_queries(qs)
    cap = 64 << 20
    buf = C.create_string_buffer(cap)
    f_one = s._f("list")
    f_batch = s._f("list_batch")

    def run_loop():
        out_len = C.c_size_t(); hr = C.c_uint64(); more = C.c_int()
        cnt = C.cast(buf, C.POINTER(C.c_uint32))
        kvs = nbytes = 0
        t0 = time.perf_counter()
        for st, en, rev, lim in qs:
            rc = f_one(h, st, C.c_size_t(len(st)), en, C.c_size_t(len(en)),
                       C.c_uint64(rev), C.c_int64(lim), buf, C.c_size_t(cap),
                       C.byref(out_len), C.byref(hr), C.byref(more))
            assert rc == OK, rc
            kvs += cnt[0]
            nbytes += out_len.value
        return time.perf_counter() - t0, kvs, nbytes

    def run_batch(flags):
        nonlocal buf, cap
        out_len = C.c_size_t(); total = C.c_ulonglong()
        t0 = time.perf_counter()
        while True:
            rc = f_batch(h, qbuf, C.c_size_t(len(qs)), C.c_int(flags), buf,
                         C.c_size_t(cap), C.byref(out_len), C.byref(total))
            if rc != ENOBUF:
                break
            cap = out_len.value + (out_len.value >> 2)
            buf = C.create_string_buffer(cap)   # grows in the warm-up only
        assert rc == OK, rc
        return time.perf_counter() - t0, total.value, out_len.value

    paths = {"list_loop": run_loop, "batch_full": lambda: run_batch(0),
             "batch_keys_only": lambda: run_batch(1)}
    for name in list(paths) * 2:         # warm every path twice
        paths[name]()
    rows = {name: [] for name in paths}
    counters = {"batch_full": [], "batch_keys_only": []}
    for _rnd in range(args.rounds):
        for name, fn in paths.items():
            p0 = perf(s)
            dt, kvs, nb = fn()
            p1 = perf(s)
            rows[name].append((dt, kvs, nb))
            if name in counters:
                c = {k: round(p1[k] - p0[k], 3) for k in COUNTERS}
                c["wall_ms"] = round(dt * 1e3, 3)
                counters[name].append(c)
    res = {"config": {"keys": per_ns * len(nss), "namespaces": len(nss),
                      "queries": len(qs), "limit": args.limit,
                      "value_bytes": args.value_bytes, "rounds": args.rounds}}
    for name, rs in rows.items():
        res[name] = {
            "kvs_per_round": [r[1] for r in rs],
            "reply_bytes_per_round": [r[2] for r in rs],
            "wall_ms": spread([r[0] * 1e3 for r in rs]),
            "kvs_per_sec": spread([r[1] / r[0] for r in rs]),
            "reply_bytes_per_sec": spread([r[2] / r[0] for r in rs]),
        }
    for name, cs in counters.items():
        res[name]["per_round_counters"] = cs
    for name in counters:
        # a speed-up is claimed only when the slowest batch round beats the
        # fastest loop round, i.e. the difference exceeds the measured spread
        res[name]["loop_over_batch_wall_median"] = round(
            res["list_loop"]["wall_ms"]["median"] / res[name]["wall_ms"]["median"], 2)
        res[name]["difference_exceeds_spread"] = bool(
            res[name]["wall_ms"]["max"] < res["list_loop"]["wall_ms"]["min"])
    s.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=200000)
    ap.add_argument("--namespaces", type=int, default=400)
    ap.add_argument("--queries", type=int, default=300)
    ap.add_argument("--limit", type=int, default=500)
    ap.add_argument("--value-bytes", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # the GPU step: a fresh child under its own time limit (this parent never
    # touches the GPU)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable,
           os.path.abspath(__file__), "--worker"] + sys.argv[1:]
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
