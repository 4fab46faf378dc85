"""GPU micro-benchmark of the range digest (not a pytest): one kb_digest_batch
(k_digest_plan / k_digest_tiles) against the only other way
to the same answer, kb_list_batch of the same ranges plus a host hash of the
reply (kb_test_digest_record per record).

One store per KB_DIGEST_TILE value, K keys in bench-shaped namespaces
(/registry/pods/ns-XXXX/pod-XXXXX). Per tile size: one digest call over the N
namespaces plus the whole prefix ("many") and over the whole prefix alone
("one"), warmed twice, the C call alone timed, with wall time, digest_ms and
the payload bytes per second of the two kernels. At the first tile size the
List alternative is timed too (its call, list_ms + list_d2h_ms, and the host
hash apart) and the two answers must agree.

Every store is measured in a child process under its own time limit; the
first child that fails ends the run:

    python tests/digest_batch_micro.py --out profiles/digest_batch.json
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

from count_batch_micro import load, perf, spread  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s, the figure DESIGN.md §3.3 uses


def measure_digest(s, qs, rounds):
    h = C.c_void_p(s.h)
    qbuf = s.encode_queries(qs)
    cap = 4 + 48 * len(qs)
    buf = C.create_string_buffer(cap)
    f = s._f("digest_batch")
    out_len, total = C.c_size_t(), C.c_ulonglong()
    wall, dev, bytes_ = [], [], 0
    for rnd in range(rounds + 2):            # two warm-up rounds
        p0 = perf(s)
        t0 = time.perf_counter()
        rc = f(h, qbuf, C.c_size_t(len(qs)), C.c_int(0), buf, C.c_size_t(cap),
               C.byref(out_len), C.byref(total))
        dt = time.perf_counter() - t0
        p1 = perf(s)
        assert rc == 0 and out_len.value == cap, (rc, out_len.value)
        if rnd >= 2:
            wall.append(dt * 1e3)
            dev.append(p1["digest_ms"] - p0["digest_ms"])
            bytes_ = p1["digest_batch_bytes"] - p0["digest_batch_bytes"]
            tiles = p1["digest_batch_tiles"] - p0["digest_batch_tiles"]
    bps = bytes_ / (statistics.median(dev) * 1e-3)
    return {"queries": len(qs), "kvs": total.value, "payload_bytes": bytes_,
            "tiles": tiles, "wall_ms": spread(wall), "digest_ms": spread(dev),
            "payload_bytes_per_s": round(bps, 0),
            "fraction_of_6.3TBps": round(bps / HBM_ACHIEVABLE, 4)}, \
        C.string_at(buf, cap)


def measure_list(s, qs, rounds):
    """kb_list_batch of qs, then kb_test_digest_record over every record of
    the reply -> (timings, [(count, key_bytes, value_bytes, hash)])."""
    from kubebrain_amd.client import record_digest
    wall, dev, hash_ms, ans = [], [], [], None
    for rnd in range(rounds + 1):            # one warm-up round
        p0 = perf(s)
        t0 = time.perf_counter()
        rc, res, _sec = s.list_batch(qs)
        dt = time.perf_counter() - t0        # includes the client's parse
        p1 = perf(s)
        assert rc == 0, rc
        t0 = time.perf_counter()
        ans = [(len(r.kvs), sum(len(kv.key) for kv in r.kvs),
                sum(len(kv.value) for kv in r.kvs),
                sum(record_digest(kv.revision, kv.key, kv.value) for kv in r.kvs)
                & ((1 << 64) - 1)) for _st, r in res]
        th = time.perf_counter() - t0
        if rnd >= 1:
            wall.append(dt * 1e3)
            dev.append(p1["list_ms"] + p1["list_d2h_ms"] - p0["list_ms"] - p0["list_d2h_ms"])
            hash_ms.append(th * 1e3)
    return {"list_batch_wall_ms_with_python_parse": spread(wall),
            "list_ms_plus_list_d2h_ms": spread(dev),
            "host_hash_ms_python_ctypes": spread(hash_ms)}, ans


def worker(args):
    import struct
    rows = 2 * args.keys + (1 << 20)
    os.environ.setdefault("KB_MAX_ROWS", str(max(4 << 20, rows)))
    os.environ.setdefault("KB_HEAP_BYTES", str(max(1 << 30, 2 * rows * args.value_bytes)))
    os.environ.setdefault("KB_FLUSH_ROWS", "262144")
    os.environ.setdefault("KB_EVENT_LOG", "0")
    s, nss, per_ns = load(args.keys, args.namespaces, args.value_bytes)
    whole = (b"/registry/pods/", b"/registry/pods0", 0, 0)
    many = [(ns + b"/", ns + b"0", 0, 0) for ns in nss] + [whole]
    res = {"digest_tile": int(os.environ["KB_DIGEST_TILE"])}
    res["many"], raw = measure_digest(s, many, args.rounds)
    res["one"], _ = measure_digest(s, [whole], args.rounds)
    if args.with_list:
        res["list_alternative_namespaces"], ans = measure_list(s, many[:-1], 2)
        got = [struct.unpack_from("<QQQQ", raw, 4 + 48 * i + 16) for i in range(len(nss))]
        assert got == ans, "digest and List + host hash disagree"
        res["answers_agree"] = True
    p = perf(s)
    res["base_rows"], res["delta_rows"] = p["base_rows"], p["delta_rows"]
    s.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=200000)
    ap.add_argument("--namespaces", type=int, default=400)
    ap.add_argument("--value-bytes", type=int, default=512)
    ap.add_argument("--tiles", default="1024,256,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--with-list", action="store_true")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # the GPU steps: fresh children under their own time limits (this parent
    # never touches the GPU); nothing more is started after one fails
    res = {"config": {"keys": args.keys, "namespaces": args.namespaces,
                      "value_bytes": args.value_bytes, "rounds": args.rounds},
           "by_tile": []}
    for i, tile in enumerate(args.tiles.split(",")):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable,
               os.path.abspath(__file__), "--worker", "--keys", str(args.keys),
               "--namespaces", str(args.namespaces), "--value-bytes",
               str(args.value_bytes), "--rounds", str(args.rounds)]
        if i == 0:
            cmd.append("--with-list")
        out = subprocess.run(cmd, env=dict(os.environ, KB_DIGEST_TILE=tile),
                             capture_output=True, text=True)
        if out.returncode != 0:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            sys.exit(out.returncode)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res["by_tile"].append(json.loads(line[7:]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
