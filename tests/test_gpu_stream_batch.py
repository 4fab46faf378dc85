"""GPU tests for kb_stream_next_batch: a stream's next kvs found, merged and
serialized by the k_stream_* kernels window by window.

Reference for every case: the ORACLE's unbounded list(start, end, read_rev),
serialized in Python to the kb_list wire and compared as a whole with the
concatenated records of all replies. The whole-stream cases also assert from
kb_perf_json that every call took the device path (no k_range_scan2 launch, no
host record) and that the rows the mark kernel covered stay linear in the rows
of the range.
"""
import ctypes as C
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import benchwire as bw
import parity
import test_gpu_bench_records as tbr
from kbclient import COMPACTED, ENOBUF, INVALID_ARG, OK

pytestmark = pytest.mark.gpu

parity.small_env()

WHOLE = (b"/registry/", b"/registry0")
DEFAULT_WINDOW = 1 << 18


def wire(kvs, konly=False):
    return b"".join(struct.pack("<QI", r, len(k)) + k +
                    (struct.pack("<I", 0) if konly else struct.pack("<I", len(v)) + v)
                    for r, k, v in kvs)


def reference(d, rng, rev, cache):
    key = (rng, rev)
    if key not in cache:
        lo = d.o.list(rng[0], rng[1], rev, 0)
        assert lo.status == OK
        cache[key] = [(kv.revision, kv.key, kv.value) for kv in lo.kvs]
    return cache[key]


def drain(p, sid, max_kvs, flags, lib_max=65536):
    """kb_stream_next_batch until the end marker, every reply held to the
    contract. -> (record bytes of all replies, calls made)."""
    recs, calls, ended = b"", 0, False
    while True:
        rc, raw, more, n, out_len = p.stream_next_batch(sid, max_kvs, flags)
        calls += 1
        assert rc == OK, (rc, bw._err(p))
        assert out_len == len(raw) <= p.BUF and struct.unpack_from("<I", raw)[0] == n
        assert n <= (max_kvs if 0 < max_kvs <= lib_max else lib_max)
        if n == 0:                       # empty only as the last reply
            assert more == 0 and raw == b"\x00" * 4
            break
        assert not ended                 # more == 0 was the last non-empty one
        ended = more == 0
        recs += raw[4:]
    assert p.stream_next_batch(sid, max_kvs, flags)[0] == INVALID_ARG   # freed
    return recs, calls


def add_delta(d, info):
    """Rows left in the delta over the flushed base: newer revisions that
    shadow base rows, tombstones of base keys, fresh keys between base keys."""
    keys, rev, dead = info["keys"], info["rev"], set(info["dead"])
    live = [k for k in keys[:tbr.PER_NS * 6] if k not in dead]
    for i, k in enumerate(live[5:400:9]):
        r = d.update(k, tbr.val(i + 900, tbr.VLENS[i % 8]), rev[k])
        assert r.succeeded
        rev[k] = r.header_revision
    for k in live[7:400:23]:
        assert d.delete(k, rev[k]).succeeded
    for i, k in enumerate(live[2:400:31] + tbr.LONG[1:3]):
        assert d.create(k + b"-new", tbr.val(i + 77, 33)).succeeded
    d.count(*WHOLE)                                          # device state current


@pytest.fixture(scope="module", params=[(w, st) for w in (64, 192, None)
                                        for st in ("delta", "flushed")],
                ids=lambda p: "w%s-%s" % p)
def world(request):
    """The bench-records fixture store (~3000 rows), flushed, plus add_delta's
    rows; `flushed` folds those too, so the delta run is empty."""
    window, state = request.param
    knobs = {"KB_STREAM_WINDOW": window} if window else {}
    d = bw.open_dual(**knobs)
    try:
        info = tbr.build(d)
        bw.flush(d.p)
        add_delta(d, info)
        if state == "flushed":
            bw.flush(d.p)
        p = bw.perf(d.p)
        assert p["base_rows"] > 2500 and (p["delta_rows"] > 60) == (state == "delta"), p
        yield d, info, window or DEFAULT_WINDOW, {}
    finally:
        d.close()


# ---- 1 + 5. whole stream, and the path it took -------------------------------
@pytest.mark.parametrize("max_kvs", [1, 7, 300, 0])
@pytest.mark.parametrize("konly", [0, 1])
@pytest.mark.parametrize("mid", [False, True])
def test_whole_stream(world, max_kvs, konly, mid):
    d, info, window, cache = world
    rev = info["hist"][1] if mid else 0
    st, sid, read_rev = d.p.stream_open(*WHOLE, rev)
    assert st == OK and read_rev == (rev or d.o.current_rev())
    want = reference(d, WHOLE, read_rev, cache)
    before = bw.perf(d.p)
    recs, calls = drain(d.p, sid, max_kvs, konly)
    after = bw.perf(d.p)
    assert recs == wire(want, konly)
    assert len(want) > 1000 and calls >= -(-len(want) // (max_kvs or 65536)) + 1
    dl = {k: after[k] - before[k] for k in after if k.startswith(("stream_batch", "scan_l"))}
    assert dl["stream_batch_calls"] == calls and dl["scan_launches"] == 0, dl
    assert dl["stream_batch_host"] == 0 and dl["stream_batch_kvs"] == len(want), dl
    rows = after["base_rows"] + after["delta_rows"]          # the range is the store
    assert dl["stream_batch_rows"] <= rows + calls * (window + after["delta_rows"]), dl
    assert dl["stream_batch_windows"] >= after["base_rows"] // window, dl


# ---- 2. boundaries -----------------------------------------------------------
@pytest.fixture(scope="module")
def edges():
    """Window 64: a key of 70 base revisions and one more in the delta, keys of
    97..300 B tying on the 96-byte prefix, runs of rows without any winner."""
    ns = b"/registry/ed"
    d = bw.open_dual(KB_STREAM_WINDOW=64, KB_FLUSH_ROWS=100000)
    try:
        hot, hot_revs = ns + b"/b-hot", []
        for i in range(20):
            d.create(ns + b"/a-%03d" % i, tbr.val(i, 40))
        r = d.create(hot, b"v0").header_revision
        for i in range(69):
            hot_revs.append(r)
            r = d.update(hot, tbr.val(i, 17 + i), r).header_revision
        hot_revs.append(r)
        gone = {}
        for i in range(80):                                  # tombstoned below
            gone[ns + b"/c-%03d" % i] = d.create(ns + b"/c-%03d" % i, b"x").header_revision
        p96 = ns + b"/l-" + b"y" * (96 - len(ns) - 3)
        longs = [p96 + bytes([0x61 + i % 7]) * (1 + (i * 29) % 204) for i in range(40)]
        lrev = {k: d.create(k, tbr.val(i, 50)).header_revision for i, k in enumerate(sorted(set(longs)))}
        for k, r0 in gone.items():
            assert d.delete(k, r0).succeeded
        mid = d.p.current_rev()
        for i in range(40):                                  # above `mid`
            d.create(ns + b"/d-%03d" % i, tbr.val(i, 9))
        bw.flush(d.p)
        base_cur = d.p.current_rev()
        hot_revs.append(d.update(hot, b"newest-in-delta", hot_revs[-1]).header_revision)
        for i, (k, r0) in enumerate(sorted(lrev.items())[::3]):
            assert (d.delete(k, r0) if i % 2 else d.update(k, b"dl", r0)).succeeded
        d.count(ns + b"/", ns + b"0")
        p = bw.perf(d.p)
        assert p["base_rows"] > 400 and p["delta_rows"] > 10, p
        assert len(p96) == 96 and {len(k) for k in lrev} >= {97, 300}
        yield d, (ns + b"/", ns + b"0"), hot_revs[::6] + [hot_revs[-2], mid, base_cur, 0], {}
    finally:
        d.close()


@pytest.mark.parametrize("max_kvs", [0, 3])
@pytest.mark.parametrize("ri", range(16))
def test_window_boundaries(edges, ri, max_kvs):
    d, rng, revs, cache = edges
    assert len(revs) == 16
    st, sid, read_rev = d.p.stream_open(*rng, revs[ri])
    assert st == OK
    want = reference(d, rng, read_rev, cache)
    before = bw.perf(d.p)
    recs, calls = drain(d.p, sid, max_kvs, 0)
    assert recs == wire(want) and len(want) >= 20
    assert bw.perf(d.p)["stream_batch_windows"] - before["stream_batch_windows"] >= 7


# ---- 3. buffer and flags -----------------------------------------------------
def raw_call(p, sid, max_kvs, flags, cap, slack=64):
    buf = C.create_string_buffer(b"\xc3" * (cap + slack), cap + slack)
    out_len, n, more = C.c_size_t(), C.c_ulonglong(), C.c_int()
    rc = p._f("stream_next_batch")(C.c_void_p(p.h), C.c_longlong(sid),
                                   C.c_longlong(max_kvs), C.c_int(flags), buf,
                                   C.c_size_t(cap), C.byref(out_len), C.byref(n),
                                   C.byref(more))
    mem = C.string_at(buf, cap + slack)
    return rc, out_len.value, n.value, mem[:cap], mem[cap:] == b"\xc3" * slack


@pytest.mark.parametrize("k", [1, 3, 40])
def test_buffer(world, k):
    d, info, _window, cache = world
    st, sid, read_rev = d.p.stream_open(*WHOLE, 0)
    want = reference(d, WHOLE, read_rev, cache)
    sizes = [16 + len(key) + len(v) for _r, key, v in want]
    for flags in (2, 3, -2, 1 << 20):                        # only bit 0 is a flag
        assert raw_call(d.p, sid, 0, flags, 64) == (INVALID_ARG, 0, 0, b"\xc3" * 64, True)
    for cap in (0, 3, 4, 4 + sizes[0] - 1):                  # below the first record
        rc, out_len, n, mem, ok = raw_call(d.p, sid, 0, 0, cap)
        assert (rc, out_len, n, mem, ok) == (ENOBUF, 4 + sizes[0], 0, b"\xc3" * cap, True), cap
    cap = 4 + sum(sizes[:k])                                 # exactly k records
    rc, out_len, n, mem, ok = raw_call(d.p, sid, 0, 0, cap)
    assert (rc, out_len, n, ok) == (OK, cap, k, True)
    assert mem == struct.pack("<I", k) + wire(want[:k])
    rc, out_len, n, mem, ok = raw_call(d.p, sid, 0, 0, 4 + sizes[k] - 1)
    assert (rc, out_len, n, ok) == (ENOBUF, 4 + sizes[k], 0, True)
    recs, _ = drain(d.p, sid, 500, 0)                        # that record comes first
    assert recs == wire(want[k:])


# ---- 4. interleaving ---------------------------------------------------------
def test_interleaved_with_stream_next_and_writes():
    ns = b"/registry/il"
    rng = (ns + b"/", ns + b"0")
    d = bw.open_dual(KB_STREAM_WINDOW=256, KB_FLUSH_ROWS=100000)
    try:
        keys = [ns + b"/k-%04d" % i for i in range(1500)]
        revs = []
        for c0 in range(0, len(keys), 500):
            revs += bw.dual_txn(d, [(k, 0, tbr.val(i, 30 + i % 50)) for i, k in
                                    enumerate(keys[c0:c0 + 500])])
        bw.flush(d.p)
        cur = dict(zip(keys, revs))
        upd = bw.dual_txn(d, [(k, cur[k], b"second") for k in keys[::7]])
        assert all(upd)
        cur.update(zip(keys[::7], upd))
        st, sid, read_rev = d.p.stream_open(*rng, 0)
        assert st == OK
        want = [(kv.revision, kv.key, kv.value) for kv in d.o.list(*rng, read_rev, 0).kvs]
        got, step, done = b"", 0, False
        while not done:
            if step % 2:
                rc, raw = d.p.stream_next(sid)
            else:
                rc, raw, _more, _n, _ = d.p.stream_next_batch(sid, 170)
            assert rc == OK
            done = raw == b"\x00" * 4
            got += raw[4:]
            k = keys[(step * 97) % len(keys)]                # writes inside the range
            r = d.update(k, b"later-%d" % step, cur[k])
            assert r.succeeded
            cur[k] = r.header_revision
            assert d.create(k + b"-fresh-%d" % step, b"new").succeeded
            if step == 2:
                bw.flush(d.p)
            if step in (1, 4):
                bw.bench_step(d.p, [rng + (0, 10)], [], 4)   # left in flight
            step += 1
        assert got == wire(want) and step >= 6
        bw.sync(d.p)
    finally:
        d.close()


def test_compacted_mid_stream():
    ns = b"/registry/cm"
    rng = (ns + b"/", ns + b"0")
    d = bw.open_dual()
    try:
        for i in range(40):
            d.create(ns + b"/k-%02d" % i, b"v%d" % i)
        sids = [d.p.stream_open(*rng, 0)[1] for _ in range(2)]
        for sid in sids:
            assert d.p.stream_next_batch(sid, 5)[3] == 5
        d.update(ns + b"/k-00", b"w", 0)
        assert d.compact(d.p.current_rev())[0] == OK         # past read_rev
        assert d.p.stream_next_batch(sids[0], 5)[0] == COMPACTED
        assert d.p.stream_next(sids[1])[0] == COMPACTED
        for sid in sids:                                     # gone for both calls
            assert d.p.stream_next_batch(sid, 5)[0] == INVALID_ARG
            assert d.p.stream_next(sid)[0] == INVALID_ARG
    finally:
        d.close()
