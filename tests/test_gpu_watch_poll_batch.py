"""GPU tests for kb_watch_poll_batch: n watchers polled in one call, their
sections serialized on the device from the payload ring (k_wpoll_size /
k_wpoll_emit).

Reference for every section: the ORACLE's okb_watch_poll for the same
watcher. Parsed events must be equal and the raw section bytes must equal a
Python re-serialization of the oracle's events. Device-path cases also
assert from kb_perf_json that the kernels served exactly the events returned
(wpoll_events_dev) and that nothing fell back to the host serializer
(wpoll_events_host == 0), so a silent fallback cannot pass.
"""
import ctypes as C
import json
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import kbclient
import parity
from kbclient import ENOBUF, INVALID_ARG, OK, WATCH_DROPPED

pytestmark = pytest.mark.gpu

parity.small_env()

VLENS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 511, 512, 513]


@pytest.fixture(autouse=True)
def _payload_env(monkeypatch):
    # a byte ring small enough to allocate instantly; cases that need another
    # size (or the default) set their own before opening the store
    monkeypatch.setenv("KB_WATCH_PAYLOAD_BYTES", str(8 << 20))
    yield monkeypatch


def ser(evs):
    out = [struct.pack("<I", len(evs))]
    for e in evs:
        out.append(struct.pack("<iQQI", e.type, e.revision, e.kv_revision,
                               len(e.key)))
        out.append(e.key)
        out.append(struct.pack("<I", len(e.value)))
        out.append(e.value)
    return b"".join(out)


def perf(store):
    buf = C.create_string_buffer(4096)
    rc = store._f("perf_json")(C.c_void_p(store.h), buf, C.c_size_t(4096))
    assert rc == 0
    return json.loads(buf.value.decode())


def perf_reset(store):
    store._f("perf_reset")(C.c_void_p(store.h))


def last_error(store):
    buf = C.create_string_buffer(512)
    code = store.lib.kb_last_error(buf, C.c_size_t(512))
    return code, buf.value.decode(errors="replace")


def arm(d):
    rc, res, raw = d.p.watch_poll_batch([])
    assert (rc, res, raw) == (OK, [], [])


def batch(d, idxs):
    """Batch-poll the product for watches idxs, poll the oracle one by one,
    assert equality of events and raw bytes; returns the per-watcher events."""
    exp = [d.o.watch_poll(d.watches[i][0]) for i in idxs]
    rc, res, raw = d.p.watch_poll_batch([d.watches[i][1] for i in idxs])
    assert rc == OK, (rc, last_error(d.p))
    assert len(res) == len(raw) == len(idxs)
    for k, i in enumerate(idxs):
        so, eo = exp[k]
        sp, ep = res[k]
        assert so == sp == OK, (i, so, sp)
        assert len(eo) == len(ep), (i, len(eo), len(ep))
        assert eo == ep, (i, next((a, b) for a, b in zip(eo, ep) if a != b))
        assert raw[k] == ser(eo), i
    return [e for _, e in res]


def batch_dev(d, idxs):
    """batch() that must have been served by the kernels alone."""
    perf_reset(d.p)
    evs = batch(d, idxs)
    n = sum(len(e) for e in evs)
    p = perf(d.p)
    assert p["wpoll_events_dev"] == n, (p["wpoll_events_dev"], n)
    assert p["wpoll_events_host"] == 0, p["wpoll_events_host"]
    if n:
        assert p["wpoll_launches"] == 2 and p["wpoll_bytes"] > 0
    return evs


def batch_host(d, idxs):
    """batch() that must have been served by the host serializer alone."""
    perf_reset(d.p)
    evs = batch(d, idxs)
    n = sum(len(e) for e in evs)
    p = perf(d.p)
    assert p["wpoll_events_host"] == n, (p["wpoll_events_host"], n)
    assert p["wpoll_events_dev"] == 0, p["wpoll_events_dev"]
    return evs


def long_key(base, total):
    return base + b"k" * (total - len(base))


def mixed_writes(d, n, nss, seed=1, vlens=VLENS, extra_keys=()):
    """n successful writes (create / update / delete mix), one event each."""
    rng = random.Random(seed)
    live = d.__dict__.setdefault("_live", {})   # key -> latest revision
    keys = [ns + b"/obj-%04d" % i for ns in nss for i in range(40)]
    keys += list(extra_keys)
    done = 0
    while done < n:
        key = keys[rng.randrange(len(keys))]
        val = bytes([65 + done % 26]) * vlens[done % len(vlens)]
        if key not in live:
            r = d.create(key, val)
            if r.succeeded:
                live[key] = r.header_revision
        elif rng.random() < 0.25:
            r = d.delete(key, live[key])
            if r.succeeded:
                del live[key]
        else:
            r = d.update(key, val, live[key])
            if r.succeeded:
                live[key] = r.header_revision
        assert r.succeeded, key
        done += 1


NSS = [b"/registry/pods/ns-%02d" % i for i in range(6)]


# ---- 1. basic fan-out ------------------------------------------------------

def test_basic_fanout(_payload_env):
    _payload_env.delenv("KB_WATCH_PAYLOAD_BYTES")  # the 256 MiB default
    d = parity.Dual()
    try:
        arm(d)
        lk = [long_key(b"/registry/pods/ns-long/", n) for n in (95, 96, 97, 300)]
        prefixes = [b"/registry/"] + [ns + b"/" for ns in NSS]
        prefixes += [ns + b"/obj-00%d" % j for ns in NSS for j in range(4)]
        prefixes += [b"/registry/pods/ns-long/", lk[0], lk[1][:96], lk[3][:90]]
        prefixes += [b"/registry/nothing/"]
        while len(prefixes) < 70:
            prefixes.append(NSS[len(prefixes) % 6] + b"/obj-001%d" % (len(prefixes) % 10))
        assert len(prefixes) == 70
        idxs = [d.watch(p, 0) for p in prefixes]
        mixed_writes(d, 700, NSS, seed=3, extra_keys=lk)
        evs = batch_dev(d, idxs)
        assert len(evs[0]) == 700
        assert evs[prefixes.index(b"/registry/nothing/")] == []
        assert len(evs[prefixes.index(b"/registry/pods/ns-long/")]) > 0
        assert {len(e.value) for e in evs[0] if e.type != 2} >= set(VLENS)
        assert {95, 96, 97, 300} <= {len(e.key) for e in evs[0]}
        # drained: a second poll returns all-empty sections
        rc, res, raw = d.p.watch_poll_batch([d.watches[i][1] for i in idxs])
        assert rc == OK
        assert all(st == OK and e == [] for st, e in res)
        assert all(s == b"\0\0\0\0" for s in raw)
        d.diff_event_log()
    finally:
        d.close()


# ---- 2. interleaving with kb_watch_poll --------------------------------------

def test_interleaved_with_single_poll():
    d = parity.Dual()
    try:
        arm(d)
        idxs = [d.watch(p, 0) for p in
                [b"/registry/"] + [ns + b"/" for ns in NSS] + [NSS[0] + b"/obj-000"]]
        a, b = idxs[:4], idxs[4:]
        for rnd in range(3):
            mixed_writes(d, 150, NSS, seed=10 + rnd)
            for i in a:
                d.poll(i)          # kb_watch_poll vs the oracle
            batch_dev(d, b)        # batch vs the oracle
            a, b = b, a
        d.diff_event_log()
    finally:
        d.close()


# ---- 3. ENOBUF ---------------------------------------------------------------

def raw_batch(store, wids, cap, canary=0xA5):
    buf = (C.c_ubyte * (cap + 64))(*([canary] * (cap + 64)))
    arr = (C.c_longlong * max(len(wids), 1))(*wids)
    out_len = C.c_size_t(); total = C.c_ulonglong()
    rc = store._f("watch_poll_batch")(C.c_void_p(store.h), arr,
                                      C.c_size_t(len(wids)), buf,
                                      C.c_size_t(cap), C.byref(out_len),
                                      C.byref(total))
    return rc, out_len.value, bytes(buf), total.value


def test_enobuf_drains_nothing():
    d = parity.Dual()
    try:
        arm(d)
        idxs = [d.watch(p, 0) for p in [b"/registry/", NSS[0] + b"/", NSS[1] + b"/",
                                        b"/registry/nothing/", NSS[2] + b"/obj-00"]]
        mixed_writes(d, 120, NSS[:3], seed=5)
        exp = [d.o.watch_poll(d.watches[i][0])[1] for i in idxs]
        secs = [ser(e) for e in exp]
        wids = [d.watches[i][1] for i in idxs]
        req = 4 + sum(8 + len(s) for s in secs)
        for cap in (0, 3, req - 1):
            rc, need, buf, _ = raw_batch(d.p, wids, cap)
            assert rc == ENOBUF and need == req, (cap, rc, need, req)
            if cap < 4:
                assert buf == b"\xA5" * len(buf)       # canary untouched
            assert buf[cap:] == b"\xA5" * 64           # never past cap
        # a single kb_watch_poll after the failed batches still sees everything
        rc, evs = d.p.watch_poll(wids[0])
        assert rc == OK and evs == exp[0] and len(evs) == 120
        req2 = req - (len(secs[0]) - 4)
        rc, need, _, _ = raw_batch(d.p, wids, req2 - 1)
        assert rc == ENOBUF and need == req2
        # the retry with the exact size returns every event
        perf_reset(d.p)
        rc, need, buf, total = raw_batch(d.p, wids, req2)
        assert rc == OK and need == req2
        want = struct.pack("<I", len(wids))
        for k, s in enumerate(secs):
            s = b"\0\0\0\0" if k == 0 else s
            want += struct.pack("<iI", OK, len(s)) + s
        assert buf[:req2] == want
        assert buf[req2:] == b"\xA5" * 64
        assert total == sum(len(e) for e in exp[1:])
        p = perf(d.p)
        assert p["wpoll_events_dev"] == total and p["wpoll_events_host"] == 0
    finally:
        d.close()


# ---- 4. statuses -----------------------------------------------------------------

def test_dropped_and_duplicate_wids():
    d = parity.Dual()
    try:
        arm(d)
        i0 = d.watch(NSS[0] + b"/", 0)
        ic = d.watch(NSS[0] + b"/", 0)
        i1 = d.watch(b"/registry/", 0)
        mixed_writes(d, 60, NSS[:2], seed=8)
        wo_c, wp_c = d.watches[ic]
        d.o.watch_cancel(wo_c)
        d.p.watch_cancel(wp_c)
        w0, w1 = d.watches[i0][1], d.watches[i1][1]
        # duplicate wid: EINVALID, nothing drained
        rc, need, buf, _ = raw_batch(d.p, [w0, w1, w0], 1 << 16)
        assert rc == INVALID_ARG
        assert buf == b"\xA5" * len(buf)
        # cancelled + never-issued wids: DROPPED, len 0, neighbours unaffected
        e0 = d.o.watch_poll(d.watches[i0][0])[1]
        e1 = d.o.watch_poll(d.watches[i1][0])[1]
        perf_reset(d.p)
        rc, res, raw = d.p.watch_poll_batch([w0, wp_c, w1, 987654321])
        assert rc == OK
        assert res[0] == (OK, e0) and raw[0] == ser(e0)
        assert res[1] == (WATCH_DROPPED, []) and raw[1] == b""
        assert res[2] == (OK, e1) and raw[2] == ser(e1) and len(e1) == 60
        assert res[3] == (WATCH_DROPPED, []) and raw[3] == b""
        p = perf(d.p)
        assert p["wpoll_events_dev"] == len(e0) + len(e1)
        assert p["wpoll_events_host"] == 0
    finally:
        d.close()


def test_slow_consumer_dropped_product_only():
    d = parity.Dual(watch_cache_size=2048)
    try:
        arm(d)
        slow = d.watch(b"/registry/", 0)     # never polled
        fast = d.watch(b"/registry/", 0)     # polled every 300
        rng = random.Random(4)
        revs = {}
        for step in range(4000):
            key = NSS[step % 3] + b"/obj-%04d" % rng.randrange(50)
            r = d.update(key, b"v%05d" % step, revs.get(key, 0))
            assert r.succeeded
            revs[key] = r.header_revision
            if step % 300 == 299:
                batch_dev(d, [fast])
        # product only: the oracle's bound differs, so its `slow` is not asked
        e_fast = d.o.watch_poll(d.watches[fast][0])[1]
        perf_reset(d.p)
        rc, res, raw = d.p.watch_poll_batch([d.watches[slow][1],
                                             d.watches[fast][1]])
        assert rc == OK
        assert res[0] == (WATCH_DROPPED, []) and raw[0] == b""
        assert res[1] == (OK, e_fast) and raw[1] == ser(e_fast)
        assert perf(d.p)["wpoll_events_host"] == 0
        # erased: asking again is DROPPED too, by either call
        rc, res, _ = d.p.watch_poll_batch([d.watches[slow][1]])
        assert rc == OK and res[0] == (WATCH_DROPPED, [])
        assert d.p.watch_poll(d.watches[slow][1])[0] == WATCH_DROPPED
        # its device slot is free again: a new watch works and is exact
        nw = d.watch(NSS[0] + b"/", 0)
        for step in range(40):
            key = NSS[step % 3] + b"/obj-%04d" % step
            r = d.update(key, b"w%05d" % step, revs.get(key, 0))
            revs[key] = r.header_revision
        evs = batch_dev(d, [nw, fast])
        assert len(evs[1]) == 40 and 0 < len(evs[0]) < 40
    finally:
        d.close()


# ---- 5. both rings wrap ------------------------------------------------------------

def test_rings_wrap(_payload_env):
    _payload_env.setenv("KB_WATCH_PAYLOAD_BYTES", "65536")
    d = parity.Dual(watch_cache_size=2048)
    try:
        arm(d)
        w_all = d.watch(b"/registry/", 0)
        w_ns = d.watch(NSS[1] + b"/", 0)
        revs = {}
        rng = random.Random(6)
        seen = 0
        for step in range(5000):
            key = NSS[step % 4] + b"/obj-%04d" % rng.randrange(80)
            val = bytes([97 + step % 26]) * (96 + step % 9)
            r = d.update(key, val, revs.get(key, 0))
            assert r.succeeded
            revs[key] = r.header_revision
            if step % 300 == 299:
                evs = batch_dev(d, [w_all, w_ns])
                seen += len(evs[0])
        seen += len(batch_dev(d, [w_ns, w_all])[1])
        assert seen == 5000      # 2.4 event-ring laps, > 12 byte-ring laps
    finally:
        d.close()


# ---- 6. host fallbacks give identical bytes ------------------------------------------

def test_fallback_events_before_arming():
    d = parity.Dual()
    try:
        w = d.watch(b"/registry/", 0)
        w2 = d.watch(NSS[0] + b"/", 0)
        mixed_writes(d, 50, NSS[:2], seed=2)
        assert perf(d.p)["wpoll_launches"] == 0
        evs = batch_host(d, [w, w2])       # this call arms the ring
        assert len(evs[0]) == 50
        mixed_writes(d, 50, NSS[:2], seed=3)
        evs = batch_dev(d, [w, w2])
        assert len(evs[0]) == 50
    finally:
        d.close()


def test_fallback_payload_window_passed(_payload_env):
    _payload_env.setenv("KB_WATCH_PAYLOAD_BYTES", "16384")
    d = parity.Dual()                      # event ring (200k) keeps everything
    try:
        arm(d)
        lag = d.watch(b"/registry/", 0)
        near = d.watch(b"/registry/", 0)
        mixed_writes(d, 350, NSS[:2], seed=9, vlens=[100])
        batch(d, [near])
        mixed_writes(d, 20, NSS[:2], seed=11, vlens=[100])
        # `lag` holds 370 events, ~60 KB: its oldest left the 16 KiB byte ring
        perf_reset(d.p)
        evs = batch(d, [lag, near])
        p = perf(d.p)
        assert len(evs[0]) == 370 and len(evs[1]) == 20
        assert p["wpoll_events_host"] == 370 and p["wpoll_events_dev"] == 20
    finally:
        d.close()


def test_fallback_value_larger_than_ring(_payload_env):
    _payload_env.setenv("KB_WATCH_PAYLOAD_BYTES", "16384")
    d = parity.Dual()
    try:
        arm(d)
        w = d.watch(b"/registry/", 0)
        assert d.create(NSS[0] + b"/small-0", b"s" * 40).succeeded
        assert d.create(NSS[0] + b"/big", b"B" * 20000).succeeded
        evs = batch_host(d, [w])           # window emptied through the big one
        assert [len(e.value) for e in evs[0]] == [40, 20000]
        assert d.create(NSS[0] + b"/small-1", b"t" * 41).succeeded
        evs = batch_dev(d, [w])
        assert [len(e.value) for e in evs[0]] == [41]
    finally:
        d.close()


def test_fallback_long_prefix():
    d = parity.Dual()
    try:
        arm(d)
        base = long_key(b"/registry/pods/ns-long/", 120)
        wl = d.watch(base, 0)              # 120-byte prefix: exact test on host
        ws = d.watch(b"/registry/pods/ns-long/", 0)
        for j in range(12):
            # same first 96 bytes; only every other key has the full prefix
            key = (base if j % 2 else base[:110] + b"Z" * 10) + b"/%02d" % j
            assert d.create(key, b"v" * (j * 7)).succeeded
        perf_reset(d.p)
        evs = batch(d, [wl, ws])
        p = perf(d.p)
        assert len(evs[0]) == 6 and len(evs[1]) == 12
        assert p["wpoll_events_host"] == 6 and p["wpoll_events_dev"] == 12
    finally:
        d.close()


def test_fallback_payload_ring_disabled(_payload_env):
    _payload_env.setenv("KB_WATCH_PAYLOAD_BYTES", "0")
    d = parity.Dual()
    try:
        arm(d)
        idxs = [d.watch(p, 0) for p in [b"/registry/", NSS[0] + b"/", b"/registry/nothing/"]]
        mixed_writes(d, 90, NSS[:2], seed=12)
        evs = batch_host(d, idxs)
        assert len(evs[0]) == 90 and evs[2] == []
        assert perf(d.p)["wpoll_launches"] == 0
    finally:
        d.close()


# ---- 7. catch-up refs ----------------------------------------------------------------

def test_catchup_refs_through_batch():
    d = parity.Dual()
    try:
        arm(d)
        w_all = d.watch(b"/registry/", 0)
        mixed_writes(d, 130, NSS[:3], seed=13)
        first = batch_dev(d, [w_all])[0]
        mid = first[40].revision
        # registered at a historical revision: WatchCatchup refs over the
        # resident ring, delivered through the batch
        w_hist = d.watch(NSS[1] + b"/", mid)
        w_hist_all = d.watch(b"/registry/", mid)
        mixed_writes(d, 30, NSS[:3], seed=14)
        evs = batch_dev(d, [w_hist, w_all, w_hist_all])
        assert len(evs[2]) == 90 + 30 and len(evs[1]) == 30
        assert 0 < len(evs[0]) < 120
    finally:
        d.close()


# ---- 8. seeded soak ----------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0x6B62, 0xBEEF, 17])
def test_seeded_soak(seed):
    d = parity.Dual()
    try:
        arm(d)
        rng = random.Random(seed)
        prefixes = [b"/registry/"] + [ns + b"/" for ns in NSS] + \
                   [NSS[0] + b"/obj-000", NSS[1] + b"/obj-001", NSS[2] + b"/obj-0",
                    b"/registry/nothing/", NSS[5] + b"/obj-003"]
        idxs = [d.watch(p, 0) for p in prefixes]
        assert len(idxs) == 12
        live = {}
        for step in range(1500):
            op = rng.random()
            key = rng.choice(NSS) + b"/obj-%04d" % rng.randrange(40)
            val = bytes([65 + step % 26]) * rng.choice(VLENS)
            if op < 0.4:
                r = d.create(key, val)
                if r.succeeded:
                    live[key] = r.header_revision
            elif op < 0.75:
                prev = live.get(key, 0) if rng.random() < 0.8 else rng.randrange(1, 3000)
                r = d.update(key, val, prev)
                if r.succeeded:
                    live[key] = r.header_revision
            elif op < 0.9:
                r = d.delete(key, live.get(key, 0) if rng.random() < 0.6 else 0)
                if r.succeeded:
                    live.pop(key, None)
            else:
                ns = rng.choice(NSS)
                d.list(ns + b"/", ns + b"0", 0, rng.choice([0, 5, 17]))
            if step % 7 == 6:
                sub = rng.sample(idxs, rng.randrange(1, 13))
                batch_dev(d, sub)
            elif step % 50 == 49:
                d.poll(rng.choice(idxs))
        batch_dev(d, idxs)
        d.diff_event_log()
        d.diff_dump()
    finally:
        d.close()
