"""GPU micro-benchmark of the Count path (not a pytest): kb_count, one query
per call through k_range_scan2 (ONE block walks the whole range), against
kb_count_batch, whose ranges are cut into row tiles counted across the chip
(k_count_plan / k_count_tiles).

One process, one store, K keys in bench-shaped namespaces
(/registry/pods/ns-XXXX/pod-XXXXX). Two comparisons, rounds alternating
between the paths so drift hits all alike, all warmed twice, the C calls
alone timed:

  many  the N namespaces plus the whole prefix: a loop of N + 1 kb_count
        calls against ONE kb_count_batch;
  one   the whole-prefix query alone: one kb_count against one kb_count_batch
        of n = 1. Wall time and scan_ms against count_ms set the one-block
        scan against the tiled kernel.

Per path it reports wall time with the round-to-round spread and the
kb_perf_json counters per round. --big-keys K2 repeats the whole-prefix pair
on a second store of K2 keys (the benchmark's slab has 10M).

The measuring step runs in a child process under its own time limit:

    python tests/count_batch_micro.py --out profiles/count_batch.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COUNTERS = ("scan_ms", "scan_launches", "rows_scanned", "count_ms",
            "count_d2h_ms", "count_batch_q", "count_batch_launches",
            "count_batch_tiles", "count_batch_rows")


def perf(store):
    buf = C.create_string_buffer(8192)
    store._f("perf_json")(C.c_void_p(store.h), buf, C.c_size_t(8192))
    return json.loads(buf.value.decode())


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4),
            "max": round(max(xs), 4)}


def load(nkeys, namespaces, value_bytes):
    import kubebrain_amd

    s = kubebrain_amd.open_store()
    s.set_current_rev(1000)
    h = C.c_void_p(s.h)
    per_ns = nkeys // namespaces
    nss = [b"/registry/pods/ns-%04d" % i for i in range(namespaces)]
    bulk = s._f("bulk_create")
    val = b"v" * value_bytes
    for ns in nss:                       # one kb_bulk_create per namespace
        keys = [ns + b"/pod-%05d" % j for j in range(per_ns)]
        klens = (C.c_uint32 * per_ns)(*[len(k) for k in keys])
        vlens = (C.c_uint32 * per_ns)(*([value_bytes] * per_ns))
        rc = bulk(h, b"".join(keys), klens, val * per_ns, vlens, C.c_size_t(per_ns))
        assert rc == 0, rc
    return s, nss, per_ns


def measure(s, qs, rounds):
    """Alternating rounds of a kb_count loop and one kb_count_batch over qs.
    -> {path: {...}}; the counts of the two paths must agree."""
    from kubebrain_amd.client import OK

    h = C.c_void_p(s.h)
    qbuf = s.encode_queries(qs)
    cap = 4 + 24 * len(qs)
    buf = C.create_string_buffer(cap)
    f_one, f_batch = s._f("count"), s._f("count_batch")
    args = [(st, C.c_size_t(len(st)), en, C.c_size_t(len(en))) for st, en, _r, _l in qs]

    def run_loop():
        hr = C.c_uint64(); cnt = C.c_uint64()
        total = 0
        t0 = time.perf_counter()
        for st, sl, en, el in args:
            rc = f_one(h, st, sl, en, el, C.byref(hr), C.byref(cnt))
            assert rc == OK, rc
            total += cnt.value
        return time.perf_counter() - t0, total

    def run_batch():
        out_len = C.c_size_t(); total = C.c_ulonglong()
        t0 = time.perf_counter()
        rc = f_batch(h, qbuf, C.c_size_t(len(qs)), C.c_int(0), buf,
                     C.c_size_t(cap), C.byref(out_len), C.byref(total))
        dt = time.perf_counter() - t0
        assert rc == OK and out_len.value == cap, (rc, out_len.value)
        return dt, total.value

    paths = {"count_loop": run_loop, "count_batch": run_batch}
    for name in list(paths) * 2:         # warm every path twice
        paths[name]()
    rows = {name: [] for name in paths}
    counters = {name: [] for name in paths}
    for _rnd in range(rounds):
        for name, fn in paths.items():
            p0 = perf(s)
            dt, total = fn()
            p1 = perf(s)
            rows[name].append((dt, total))
            c = {k: round(p1[k] - p0[k], 4) for k in COUNTERS}
            c["wall_ms"] = round(dt * 1e3, 4)
            counters[name].append(c)
    assert len({r[1] for rs in rows.values() for r in rs}) == 1, rows
    res = {"queries": len(qs), "total_count": rows["count_loop"][0][1]}
    for name, rs in rows.items():
        res[name] = {"wall_ms": spread([r[0] * 1e3 for r in rs]),
                     "per_round_counters": counters[name]}
    res["count_loop"]["scan_ms"] = spread([c["scan_ms"] for c in counters["count_loop"]])
    res["count_batch"]["count_ms"] = spread([c["count_ms"] for c in counters["count_batch"]])
    # a speed-up is claimed only when the slowest batch round beats the
    # fastest loop round, i.e. the difference exceeds the measured spread
    res["loop_over_batch_wall_median"] = round(
        res["count_loop"]["wall_ms"]["median"] / res["count_batch"]["wall_ms"]["median"], 2)
    res["difference_exceeds_spread"] = bool(
        res["count_batch"]["wall_ms"]["max"] < res["count_loop"]["wall_ms"]["min"])
    res["scan_over_count_kernel_median"] = round(
        res["count_loop"]["scan_ms"]["median"] /
        max(res["count_batch"]["count_ms"]["median"], 1e-6), 2)
    res["kernel_difference_exceeds_spread"] = bool(
        res["count_batch"]["count_ms"]["max"] < res["count_loop"]["scan_ms"]["min"])
    return res


def worker(args):
    rows = 2 * max(args.keys, args.big_keys) + (1 << 20)
    os.environ.setdefault("KB_MAX_ROWS", str(max(4 << 20, rows)))
    os.environ.setdefault("KB_HEAP_BYTES", str(max(1 << 30, 2 * rows * 32)))
    os.environ.setdefault("KB_FLUSH_ROWS", "262144")
    os.environ.setdefault("KB_EVENT_LOG", "0")
    whole = (b"/registry/pods/", b"/registry/pods0", 0, 0)
    s, nss, per_ns = load(args.keys, args.namespaces, args.value_bytes)
    p = perf(s)
    res = {"config": {"keys": per_ns * len(nss), "namespaces": len(nss),
                      "value_bytes": args.value_bytes, "rounds": args.rounds,
                      "count_tile": int(os.environ.get("KB_COUNT_TILE", 4096)),
                      "base_rows": p["base_rows"], "delta_rows": p["delta_rows"]}}
    many = [(ns + b"/", ns + b"0", 0, 0) for ns in nss] + [whole]
    res["many"] = measure(s, many, args.rounds)
    res["one"] = measure(s, [whole], args.rounds)
    p = perf(s)
    res["config"]["base_rows"], res["config"]["delta_rows"] = p["base_rows"], p["delta_rows"]
    s.close()
    if args.big_keys:
        s, nss, per_ns = load(args.big_keys, args.big_namespaces, 16)
        big = measure(s, [whole], args.rounds)
        p = perf(s)
        big["config"] = {"keys": per_ns * len(nss), "namespaces": len(nss),
                         "value_bytes": 16, "base_rows": p["base_rows"],
                         "delta_rows": p["delta_rows"]}
        res["one_big"] = big
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
    ap.add_argument("--value-bytes", type=int, default=512)
    ap.add_argument("--big-keys", type=int, default=0)
    ap.add_argument("--big-namespaces", type=int, default=2000)
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
