"""GPU micro-benchmark of the public point-read path (not a pytest): Q keys
served by a loop of Q kb_get calls (one k_get2 launch, four small D2H copies,
a sync and a blocking value copy per call) versus ONE kb_get_batch (directory
and packed values written on the device), with values and
with no_values.

One process, one store, K keys in bench-shaped namespaces
(/registry/pods/ns-XXXX/pod-XXXXX) with V-byte values, Q of them read at the
latest revision. Rounds alternate between the paths so drift hits all alike;
all are warmed first. Only the C calls are timed; nothing is parsed into
Python objects inside the timed region. kb_get has no no_values mode, so the
no_values batch is set against the same loop. Per path it reports wall time,
gets/s and reply bytes/s with the round-to-round spread; for the batch also
the kernel and D2H time and the bytes moved (kb_perf_json get_batch_*
counters).

The measuring step runs in a child process under its own time limit:

    python tests/get_batch_micro.py --out profiles/get_batch.json
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

COUNTERS = ("get_batch_ms", "get_batch_d2h_ms", "get_batch_bytes",
            "get_batch_q_dev", "get_batch_q_host", "get_batch_found",
            "get_batch_launches", "get_launches", "get_ms")


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
    rng = np.random.default_rng(11)
    qs = [(nss[int(rng.integers(len(nss)))] + b"/pod-%05d" % int(rng.integers(per_ns)), 0)
          for _ in range(args.queries)]
    qbuf = s.encode_gets(qs)
    cap = 16 << 20
    buf = C.create_string_buffer(cap)
    f_one = s._f("get")
    f_batch = s._f("get_batch")

    def run_loop():
        hr = C.c_uint64(); has = C.c_int(); vlen = C.c_size_t(); mod = C.c_uint64()
        found = nbytes = 0
        t0 = time.perf_counter()
        for k, rev in qs:
            rc = f_one(h, k, C.c_size_t(len(k)), C.c_uint64(rev), C.byref(hr),
                       C.byref(has), buf, C.c_size_t(cap), C.byref(vlen),
                       C.byref(mod))
            assert rc == OK, rc
            found += has.value
            nbytes += vlen.value
        return time.perf_counter() - t0, found, nbytes

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

    paths = {"get_loop": run_loop, "batch_values": lambda: run_batch(0),
             "batch_no_values": lambda: run_batch(1)}
    for name in list(paths) * 2:         # warm every path twice
        paths[name]()
    rows = {name: [] for name in paths}
    counters = {name: [] for name in paths}
    for _rnd in range(args.rounds):
        for name, fn in paths.items():
            p0 = perf(s)
            dt, found, nb = fn()
            p1 = perf(s)
            rows[name].append((dt, found, nb))
            c = {k: round(p1[k] - p0[k], 3) for k in COUNTERS}
            c["wall_ms"] = round(dt * 1e3, 3)
            counters[name].append(c)
    res = {"config": {"keys": per_ns * len(nss), "namespaces": len(nss),
                      "queries": len(qs), "value_bytes": args.value_bytes,
                      "rounds": args.rounds}}
    for name, rs in rows.items():
        res[name] = {
            "found_per_round": [r[1] for r in rs],
            "reply_bytes_per_round": [r[2] for r in rs],
            "wall_ms": spread([r[0] * 1e3 for r in rs]),
            "gets_per_sec": spread([len(qs) / r[0] for r in rs]),
            "reply_bytes_per_sec": spread([r[2] / r[0] for r in rs]),
            "per_round_counters": counters[name],
        }
    for name in ("batch_values", "batch_no_values"):
        # a speed-up is claimed only when the slowest batch round beats the
        # fastest loop round, i.e. the difference exceeds the measured spread
        res[name]["loop_over_batch_wall_median"] = round(
            res["get_loop"]["wall_ms"]["median"] / res[name]["wall_ms"]["median"], 2)
        res[name]["difference_exceeds_spread"] = bool(
            res[name]["wall_ms"]["max"] < res["get_loop"]["wall_ms"]["min"])
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
    ap.add_argument("--queries", type=int, default=1024)
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
