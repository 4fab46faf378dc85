"""GPU micro-benchmark of watch registration after a reconnect storm (not a
pytest): N watchers with start revisions inside the event ring registered by
a loop of kb_watch (one catch-up scan, two stream drains and five small
copies per watcher) versus ONE kb_watch_batch (the ring staged through LDS
once per 64 watchers, three kernels per sub-batch).

One process, one store with the default 200k-event ring, filled past its
capacity with events over namespace prefixes shaped like bench.py's
(/registry/pods/ns-XXXX/). Rounds alternate between the two arms so drift
hits both alike; both are warmed first and every watcher is cancelled between
rounds. Both arms register the same (prefix, revision) list and must queue
the same number of catch-up events. Per arm it reports the wall time of the
registration with the round-to-round spread; for the batch also the kernel
time (wreg_ms) and the bytes its two read-backs moved.

The measuring step runs in a child process under its own time limit:

    python tests/watch_reg_micro.py --out profiles/watch_batch.json
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
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2),
            "max": round(max(xs), 2)}


def worker(args):
    os.environ.setdefault("KB_MAX_ROWS", str(4 << 20))
    os.environ.setdefault("KB_HEAP_BYTES", str(1 << 30))
    os.environ.setdefault("KB_FLUSH_ROWS", "262144")
    os.environ.setdefault("KB_EVENT_LOG", "0")
    import kubebrain_amd
    from kubebrain_amd.client import OK

    s = kubebrain_amd.open_store()
    s.set_current_rev(1000)
    nss = [b"/registry/pods/ns-%04d" % i for i in range(args.namespaces)]
    revs = []
    for i in range(args.events):
        r = s.create(nss[(i * 31) % len(nss)] + b"/pod-%07d" % i, b"v")
        assert r.succeeded
        revs.append(r.header_revision)
    ring = revs[-min(args.events, args.ring):]
    # start revisions spread over the resident ring, prefixes over namespaces
    watches = [(nss[(i * 7919) % len(nss)] + b"/",
                ring[(i * 104729) % len(ring)]) for i in range(args.watchers)]
    n = len(watches)
    h = C.c_void_p(s.h)
    f_one = s._f("watch")
    f_one.restype = C.c_longlong
    f_batch = s._f("watch_batch")
    f_refs = s._f("test_watch_refs")
    blob = s.encode_watches(watches)
    wids = (C.c_longlong * n)()
    sts = (C.c_int * n)()

    def pending(wid_list):
        # u32 nrefs; u64 from_rev; i64 pend_events of every watcher
        cap = 20 + 80 * (len(ring) // 512 + 2)
        head = C.create_string_buffer(cap)
        need = C.c_size_t()
        tot = 0
        for w in wid_list:
            rc = f_refs(h, C.c_longlong(w), head, C.c_size_t(cap), C.byref(need))
            assert rc == OK, rc
            tot += int.from_bytes(head.raw[12:20], "little")
        return tot

    def reg_loop():
        st = C.c_int()
        out = []
        t0 = time.perf_counter()
        for p, r in watches:
            out.append(f_one(h, p, C.c_size_t(len(p)), C.c_uint64(r), C.byref(st)))
            assert st.value == OK, st.value
        return time.perf_counter() - t0, out

    def reg_batch():
        tot = C.c_ulonglong()
        t0 = time.perf_counter()
        rc = f_batch(h, blob, C.c_size_t(len(blob)), C.c_size_t(n), C.c_int(0),
                     wids, sts, C.byref(tot))
        dt = time.perf_counter() - t0
        assert rc == OK and all(x == OK for x in sts), rc
        return dt, list(wids), tot.value

    def cancel(wid_list):
        for w in wid_list:
            s.watch_cancel(w)

    # warm both arms (first launches load code objects and size the buffers)
    _, w = reg_loop()
    want = pending(w)
    cancel(w)
    _, w, tot = reg_batch()
    assert tot == want == pending(w), (tot, want)
    cancel(w)
    rows = {"watch_loop": [], "watch_batch": []}
    counters = []
    for rnd in range(args.rounds * 2):
        if rnd % 2 == 0:
            dt, w = reg_loop()
            rows["watch_loop"].append(dt * 1e3)
        else:
            p0 = perf(s)
            dt, w, tot = reg_batch()
            p1 = perf(s)
            assert tot == want, (tot, want)
            rows["watch_batch"].append(dt * 1e3)
            c = {k: round(p1[k] - p0[k], 3) for k in
                 ("wreg_ms", "wreg_launches", "wreg_watchers_dev",
                  "wreg_events_scanned", "wreg_refs")}
            # the directory (16 B + 32 B per watcher and sub-batch) and the
            # compact ref span (80 B per ref)
            c["d2h_bytes"] = int(16 * c["wreg_launches"] / 3 + 32 * n +
                                 80 * c["wreg_refs"])
            c["wall_ms"] = round(dt * 1e3, 3)
            counters.append(c)
        cancel(w)
    res = {"config": {"watchers": n, "namespaces": args.namespaces,
                      "events_written": args.events, "ring_span": len(ring),
                      "rounds": args.rounds, "catchup_events_per_round": want},
           "watch_loop": {"register_ms": spread(rows["watch_loop"])},
           "watch_batch": {"register_ms": spread(rows["watch_batch"]),
                           "per_round_counters": counters}}
    res["loop_over_batch_median"] = round(
        res["watch_loop"]["register_ms"]["median"] /
        res["watch_batch"]["register_ms"]["median"], 2)
    # a speed-up is claimed only when the slowest batch round beats the
    # fastest loop round, i.e. the difference exceeds the measured spread
    res["difference_exceeds_spread"] = bool(
        max(rows["watch_batch"]) < min(rows["watch_loop"]))
    s.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--watchers", type=int, default=10000)
    ap.add_argument("--namespaces", type=int, default=256)
    ap.add_argument("--events", type=int, default=210000)
    ap.add_argument("--ring", type=int, default=200000,
                    help="the store's event ring capacity (its default)")
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
