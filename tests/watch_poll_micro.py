"""GPU micro-benchmark of the consumer half of the watch path (not a pytest):
draining N watchers with a loop of kb_watch_poll (host serializer, one
watcher per call) versus ONE kb_watch_poll_batch (sections serialized on the
device from the payload ring).

One process, one store, N watchers over namespace prefixes shaped like
bench.py's (/registry/pods/ns-XXXX/), rounds of W writes with V-byte values.
Rounds alternate between the two paths so drift hits both alike; both are
warmed first. Per path it reports materialized events/s and reply bytes/s
with the round-to-round spread; for the batch also the kernel time, the D2H
time and the bytes moved (kb_perf_json wpoll_* counters).

The measuring step runs in a child process under its own time limit:

    python tests/watch_poll_micro.py --out profiles/watch_poll_batch.json
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


def perf(store):
    buf = C.create_string_buffer(4096)
    store._f("perf_json")(C.c_void_p(store.h), buf, C.c_size_t(4096))
    return json.loads(buf.value.decode())


def spread(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1),
            "max": round(max(xs), 1)}


def worker(args):
    os.environ.setdefault("KB_MAX_ROWS", str(4 << 20))
    os.environ.setdefault("KB_HEAP_BYTES", str(1 << 30))
    os.environ.setdefault("KB_FLUSH_ROWS", "262144")
    os.environ.setdefault("KB_EVENT_LOG", "0")
    import kubebrain_amd
    from kubebrain_amd.client import ENOBUF, OK

    s = kubebrain_amd.open_store()
    s.set_current_rev(1000)
    nss = [b"/registry/pods/ns-%04d" % i for i in range(args.namespaces)]
    wids = []
    for i in range(args.watchers):
        st, wid = s.watch(nss[(i * 7919) % len(nss)] + b"/", 0)
        assert st == OK
        wids.append(wid)
    arr = (C.c_longlong * len(wids))(*wids)
    cap = 64 << 20
    buf = C.create_string_buffer(cap)
    f_one = s._f("watch_poll")
    f_batch = s._f("watch_poll_batch")
    h = C.c_void_p(s.h)
    revs = {}
    val = b"v" * args.value_bytes
    step = [0]

    def write_round():
        for _ in range(args.writes):
            i = step[0]
            step[0] += 1
            k = nss[i % len(nss)] + b"/pod-%05d" % (i % 4096)
            r = s.update(k, val, revs.get(k, 0))
            assert r.succeeded
            revs[k] = r.header_revision

    def drain_loop():
        nonlocal buf, cap
        out_len = C.c_size_t()
        events = nbytes = 0
        cnt = C.cast(buf, C.POINTER(C.c_uint32))
        t0 = time.perf_counter()
        for wid in wids:
            rc = f_one(h, C.c_longlong(wid), buf, C.c_size_t(cap), C.byref(out_len))
            assert rc == OK, rc
            events += cnt[0]
            nbytes += out_len.value
        return time.perf_counter() - t0, events, nbytes

    def drain_batch():
        nonlocal buf, cap
        out_len = C.c_size_t(); total = C.c_ulonglong()
        t0 = time.perf_counter()
        while True:
            rc = f_batch(h, arr, C.c_size_t(len(wids)), buf, C.c_size_t(cap),
                         C.byref(out_len), C.byref(total))
            if rc != ENOBUF:
                break
            cap = out_len.value + (out_len.value >> 2)
            buf = C.create_string_buffer(cap)   # grow once; counted in round 0
        assert rc == OK, rc
        return time.perf_counter() - t0, total.value, out_len.value

    # arm the payload ring, then warm both paths
    assert f_batch(h, arr, C.c_size_t(0), buf, C.c_size_t(cap),
                   C.byref(C.c_size_t()), C.byref(C.c_ulonglong())) == OK
    for fn in (drain_loop, drain_batch, drain_loop, drain_batch):
        write_round()
        fn()
    rows = {"poll_loop": [], "poll_batch": []}
    counters = []
    for rnd in range(args.rounds * 2):
        write_round()
        # pump outside the timed region so both paths time the drain alone
        f_batch(h, arr, C.c_size_t(0), buf, C.c_size_t(cap),
                C.byref(C.c_size_t()), C.byref(C.c_ulonglong()))
        if rnd % 2 == 0:
            dt, ev, nb = drain_loop()
            rows["poll_loop"].append((dt, ev, nb))
        else:
            p0 = perf(s)
            dt, ev, nb = drain_batch()
            p1 = perf(s)
            rows["poll_batch"].append((dt, ev, nb))
            counters.append({k: round(p1[k] - p0[k], 3) for k in
                             ("wpoll_ms", "wpoll_d2h_ms", "wpoll_bytes",
                              "wpoll_events_dev", "wpoll_events_host",
                              "wpoll_launches")})
            counters[-1]["wall_ms"] = round(dt * 1e3, 3)
    res = {"config": {"watchers": args.watchers, "namespaces": args.namespaces,
                      "writes_per_round": args.writes,
                      "value_bytes": args.value_bytes, "rounds": args.rounds}}
    for name, rs in rows.items():
        res[name] = {
            "events_per_round": [r[1] for r in rs],
            "reply_bytes_per_round": [r[2] for r in rs],
            "drain_ms": spread([r[0] * 1e3 for r in rs]),
            "events_per_sec": spread([r[1] / r[0] for r in rs]),
            "reply_bytes_per_sec": spread([r[2] / r[0] for r in rs]),
        }
    res["poll_batch"]["per_round_counters"] = counters
    lo_b = res["poll_batch"]["events_per_sec"]["min"]
    hi_l = res["poll_loop"]["events_per_sec"]["max"]
    res["batch_over_loop_median"] = round(
        res["poll_batch"]["events_per_sec"]["median"] /
        res["poll_loop"]["events_per_sec"]["median"], 2)
    # a speed-up is claimed only when the slowest batch round beats the
    # fastest loop round, i.e. the difference exceeds the measured spread
    res["difference_exceeds_spread"] = bool(lo_b > hi_l)
    s.close()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--watchers", type=int, default=10000)
    ap.add_argument("--namespaces", type=int, default=256)
    ap.add_argument("--writes", type=int, default=6000)
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
