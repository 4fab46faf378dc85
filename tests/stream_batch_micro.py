"""GPU micro-benchmark of ListByStream (not a pytest): one whole-prefix stream
over K keys with V-byte values, read by a kb_stream_next loop (300 kvs per
call through k_range_scan2, host parse and second serialization) versus a
kb_stream_next_batch loop at the default max_kvs (windows marked, merged and
serialized by the k_stream_* kernels), full values and
keys_only.

One store per KB_STREAM_WINDOW candidate, each in a child process of its own
under its own time limit, one after another. Rounds alternate between the
paths; all are warmed first. Only the C calls are timed. Per path: wall time
and kvs/s with the round-to-round spread; for the batch also the time in the
kernels and in D2H (kb_perf_json stream_batch_* counters).

    python tests/stream_batch_micro.py --out profiles/stream_batch.json
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

COUNTERS = ("stream_batch_ms", "stream_batch_d2h_ms", "stream_batch_calls",
            "stream_batch_windows", "stream_batch_rows", "stream_batch_kvs",
            "stream_batch_host", "scan_ms", "scan_launches")


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
    os.environ["KB_STREAM_WINDOW"] = str(args.window)
    import kubebrain_amd
    from kubebrain_amd.client import OK

    s = kubebrain_amd.open_store()
    s.set_current_rev(1000)
    h = C.c_void_p(s.h)
    blob = np.random.default_rng(7).integers(0x30, 0x7b, size=1 << 20,
                                             dtype=np.uint8).tobytes()
    bulk = s._f("bulk_create")
    chunk = 5000
    for c0 in range(0, args.keys, chunk):
        keys = [b"/registry/pods/ns-%04d/pod-%05d" % (j // 500, j % 500)
                for j in range(c0, min(args.keys, c0 + chunk))]
        n = len(keys)
        klens = (C.c_uint32 * n)(*[len(k) for k in keys])
        vlens = (C.c_uint32 * n)(*([args.value_bytes] * n))
        vals = b"".join(blob[37 * (j % 900):37 * (j % 900) + args.value_bytes]
                        for j in range(n))
        assert bulk(h, b"".join(keys), klens, vals, vlens, C.c_size_t(n)) == 0
    rng = (b"/registry/", b"/registry0")
    cap = 256 << 20
    buf = C.create_string_buffer(cap)
    cnt = C.cast(buf, C.POINTER(C.c_uint32))
    f_next, f_batch = s._f("stream_next"), s._f("stream_next_batch")

    def run(batch, flags=0):
        out_len = C.c_size_t(); n = C.c_ulonglong(); more = C.c_int()
        st, sid, _ = s.stream_open(*rng, 0)
        assert st == OK
        kvs = nbytes = calls = 0
        t0 = time.perf_counter()
        while True:
            if batch:
                rc = f_batch(h, C.c_longlong(sid), C.c_longlong(0), C.c_int(flags),
                             buf, C.c_size_t(cap), C.byref(out_len), C.byref(n),
                             C.byref(more))
            else:
                rc = f_next(h, C.c_longlong(sid), buf, C.c_size_t(cap),
                            C.byref(out_len))
            assert rc == OK, rc
            calls += 1
            if cnt[0] == 0:
                break
            kvs += cnt[0]
            nbytes += out_len.value
        assert kvs == args.keys, (kvs, args.keys)
        return time.perf_counter() - t0, kvs, nbytes, calls

    paths = {"next_loop": lambda: run(False), "batch_full": lambda: run(True),
             "batch_keys_only": lambda: run(True, 1)}
    for name in paths:                   # warm every path
        paths[name]()
    rows = {name: [] for name in paths}
    counters = {name: [] for name in paths}
    for _rnd in range(args.rounds):
        for name, fn in paths.items():
            p0 = perf(s)
            dt, kvs, nb, calls = fn()
            p1 = perf(s)
            rows[name].append((dt, kvs, nb))
            c = {k: round(p1[k] - p0[k], 3) for k in COUNTERS}
            c["wall_ms"], c["calls"] = round(dt * 1e3, 3), calls
            counters[name].append(c)
    res = {"window": args.window}
    for name, rs in rows.items():
        res[name] = {"wall_ms": spread([r[0] * 1e3 for r in rs]),
                     "kvs_per_sec": spread([r[1] / r[0] for r in rs]),
                     "reply_bytes": rs[0][2],
                     "per_round_counters": counters[name]}
    for name in ("batch_full", "batch_keys_only"):
        res[name]["loop_over_batch_wall_median"] = round(
            res["next_loop"]["wall_ms"]["median"] / res[name]["wall_ms"]["median"], 2)
        # a speed-up is claimed only when the ranges do not overlap
        res[name]["difference_exceeds_spread"] = bool(
            res[name]["wall_ms"]["max"] < res["next_loop"]["wall_ms"]["min"])
    s.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=200000)
    ap.add_argument("--value-bytes", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--windows", default="16384,65536,262144,1048576,4194304")
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # the GPU steps: a fresh child per window under its own time limit (this
    # parent never touches the GPU); the first failure ends the run
    out = {"config": {"keys": args.keys, "value_bytes": args.value_bytes,
                      "rounds": args.rounds}, "windows": []}
    for w in [int(x) for x in args.windows.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable,
               os.path.abspath(__file__), "--worker", "--window", str(w),
               "--keys", str(args.keys), "--value-bytes", str(args.value_bytes),
               "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit(r.returncode)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        out["windows"].append(json.loads(line[7:]))
    text = json.dumps(out, indent=1) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
