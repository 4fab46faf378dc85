"""GPU tests for kb_watch_batch: n watchers registered in one call, their
catch-up bits, pending refs and device filter rows produced by k_wreg_scan /
k_wreg_plan / k_wreg_emit.

Two references, neither of them the code under test. The ORACLE (okb_watch +
okb_watch_poll per watcher) gives the statuses and every delivered event. A
second product store, the TWIN, gets the same writes and registers the same
watchers by a loop of kb_watch; kb_test_watch_refs of every watcher must be
byte-equal between the two, and so must the watcher ids. kb_perf_json proves
that the three kernels served the catch-up entries (wreg_watchers_dev,
wreg_launches), so a silent fall-back to the kb_watch loop cannot pass.
"""
import ctypes as C
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import parity
from kbclient import ENOBUF, INVALID_ARG, OK, WATCH_EMPTY, WATCH_LOW

pytestmark = pytest.mark.gpu

parity.small_env()

L96 = b"/registry/pods/long/" + b"x" * 76          # exactly 96 bytes
NS1 = b"/registry/pods/ns-1/"
# lengths 1, 7, 8, 9, 20 (twice), 95, 96, 97 (host path) and one that matches
# nothing
PREFIXES = [b"/", b"/regist", b"/registr", b"/registry", NS1, L96[:95], L96,
            L96 + b"a", b"/registry/nomatch/", NS1]
assert [len(p) for p in PREFIXES[5:8]] == [95, 96, 97]


def key(i):
    ns = i % 5
    if ns < 3:
        return b"/registry/pods/ns-%d/p-%05d" % (ns, i)
    return L96 + (b"a" if ns == 3 else b"b") + b"-%05d" % i


def perf(store):
    buf = C.create_string_buffer(4096)
    assert store._f("perf_json")(C.c_void_p(store.h), buf, C.c_size_t(4096)) == 0
    return json.loads(buf.value.decode())


def refs(store, wid):
    """kb_test_watch_refs bytes (bound here: kbclient.py stays as it is)."""
    f = store._f("test_watch_refs")
    n = C.c_size_t()
    rc = f(C.c_void_p(store.h), C.c_longlong(wid), None, C.c_size_t(0), C.byref(n))
    assert rc == ENOBUF and n.value >= 20, (rc, n.value)
    buf = C.create_string_buffer(n.value)
    rc = f(C.c_void_p(store.h), C.c_longlong(wid), buf, n, C.byref(n))
    assert rc == OK
    return buf.raw[:n.value]


class Env:
    """Oracle + product (parity.Dual) + the twin product store."""

    def __init__(self, **kw):
        import kubebrain_amd
        self.d = parity.Dual(**kw)
        self.t = kubebrain_amd.open_store(
            store_prefix=b"/registry", watch_cache_size=kw.get("watch_cache_size", 0))
        self.t.set_current_rev(1000)
        self.revs = []     # revision of every event written, in order
        self.n = 0
        self.live = []     # (oracle wid, product wid, twin wid)

    def close(self):
        self.d.close()
        self.t.close()

    def write(self, count):
        for _ in range(count):
            k = key(self.n)
            r = self.d.create(k, b"v%d" % self.n)
            assert self.t.create(k, b"v%d" % self.n).header_revision == r.header_revision
            self.revs.append(r.header_revision)
            self.n += 1

    def churn(self, count):
        """Later traffic: updates of watched keys, new keys under the watched
        prefixes and creates outside every prefix but b"/" and its kin."""
        for j in range(count):
            if j % 3 == 2:
                k, fn = b"/registry/other/o-%05d" % self.n, "create"
            elif j % 3 == 1:
                k, fn = key(self.n), "create"
            else:
                k, fn = key(j % self.n), "update"
            self.n += fn == "create"
            r = getattr(self.d, fn)(k, b"w%d" % j)
            getattr(self.t, fn)(k, b"w%d" % j)
            if r.succeeded:
                self.revs.append(r.header_revision)

    def entries(self, nwatch, span, low=True):
        """(prefix, rev) per watcher: every prefix against start revisions 0,
        oldest, oldest - 1, newest, newest + 1 and lo at S + {0, 1, 63, 64,
        65, 511, 512}."""
        ring = self.revs[-span:]
        revs = [0, ring[0], ring[-1], ring[-1] + 1]
        revs += [ring[k] for k in (1, 63, 64, 65, 511, 512) if k < len(ring)]
        if low:
            revs.append(ring[0] - 1)
        return [(PREFIXES[i % len(PREFIXES)],
                 revs[(i // len(PREFIXES) + 3 * i) % len(revs)])
                for i in range(nwatch)], ring

    def register(self, ents, ring, reg_bytes=64 << 20):
        """Batch-register on the product, loop on oracle and twin; check
        statuses, ids, ref bytes and the perf counters."""
        d, t = self.d, self.t
        p0 = perf(d.p)
        exp = [d.o.watch(p, r) for p, r in ents]
        twin = [t.watch(p, r) for p, r in ents]
        rc, got, total = d.p.watch_batch(ents)
        assert rc == OK
        assert [s for s, _ in got] == [s for s, _ in exp] == [s for s, _ in twin]
        assert [w for _, w in got] == [w for _, w in twin]
        assert all((w == -1) == (s != OK) for s, w in got)
        new, pend = [], 0
        for (so, wo), (_, wp), (_, wt) in zip(exp, got, twin):
            if so != OK:
                continue
            a, b = refs(d.p, wp), refs(t, wt)
            assert a == b, (wp, a[:20].hex(), b[:20].hex(), len(a), len(b))
            pend += int.from_bytes(a[12:20], "little")
            new.append((wo, wp, wt))
        assert total == pend
        self.live += new
        p1 = perf(d.p)
        catch = [(p, r) for p, r in ents if ring and r and ring[0] <= r <= ring[-1]]
        n_dev = sum(len(p) <= 96 for p, _ in catch)
        assert p1["wreg_watchers_dev"] - p0["wreg_watchers_dev"] == n_dev
        assert p1["wreg_watchers_host"] - p0["wreg_watchers_host"] == len(catch) - n_dev
        assert p1["wreg_watchers_nocatchup"] - p0["wreg_watchers_nocatchup"] == \
            len(new) - len(catch)
        gwords = (len(ring) + 63) // 64
        per = max(64, reg_bytes // (8 * max(gwords, 1)))
        subs = -(-len(new) // per)
        assert p1["wreg_launches"] - p0["wreg_launches"] == 3 * subs
        return new, subs

    def poll(self, live=None):
        for wo, wp, _ in (self.live if live is None else live):
            so, eo = self.d.o.watch_poll(wo)
            sp, ep = self.d.p.watch_poll(wp)
            assert so == sp == OK, (wp, so, sp)
            assert eo == ep, (wp, len(eo), len(ep))

    def cancel(self, trip):
        for s, w in zip((self.d.o, self.d.p, self.t), trip):
            s.watch_cancel(w)
        self.live.remove(trip)


def run_case(span, nwatch, cache=0, writes=None, reg_bytes=None, low=True,
             step=530):
    e = Env(watch_cache_size=cache)
    try:
        e.write(span if writes is None else writes)
        ents, ring = e.entries(nwatch, span, low=low)
        new, subs = e.register(ents, ring, reg_bytes or (64 << 20))
        e.poll()                 # the catch-up events
        for _ in range(0, 530, step):   # more than a 512-event pump batch
            e.churn(step)
            e.poll()             # the committed table rows
        return e, new, subs
    except BaseException:
        e.close()
        raise


@pytest.mark.parametrize("span", [1, 63, 64, 65, 511, 512, 513, 1100])
def test_ring_spans(span):
    run_case(span, 130)[0].close()


@pytest.mark.parametrize("nwatch", [1, 63, 64, 65])
def test_watchers_per_call(nwatch):
    run_case(1100, nwatch)[0].close()


def test_wrapped_ring():
    # 1000 writes into a 700-event ring: the span wraps and S = 300 (mod 64 != 0)
    # (polled every 106 events: a 700-event ring drops a consumer that lags)
    run_case(700, 130, cache=700, writes=1000, step=106)[0].close()


def test_three_sub_batches(monkeypatch):
    # 1100 events = 18 grid words; 64 watchers x 18 words x 8 B per sub-batch
    monkeypatch.setenv("KB_WATCH_REG_BYTES", str(64 * 18 * 8))
    e, new, subs = run_case(1100, 130, reg_bytes=64 * 18 * 8, low=False)
    e.close()
    assert len(new) == 130 and subs == 3


def test_slot_reuse_and_interleaving():
    e, new, _ = run_case(513, 65)
    try:
        for trip in new[::2]:
            e.cancel(trip)
        e.write(70)
        ents, ring = e.entries(65, len(e.revs))
        mid = e.d.watch(b"/registry/pods/ns-0/", ring[5])   # a kb_watch in between
        assert e.t.watch(b"/registry/pods/ns-0/", ring[5])[0] == OK
        e.register(ents, ring)
        e.poll()
        e.d.poll(mid)
        e.churn(530)
        e.poll()
        e.d.poll(mid)
    finally:
        e.close()


def test_empty_ring():
    e = Env()
    try:
        ents = [(b"/", 0), (NS1, 1000), (NS1, 1001), (L96 + b"a", 5), (L96, 4000)]
        new, _ = e.register(ents, [])
        assert [s for s, _ in e.d.p.watch_batch([(b"/", 7)])[1]] == [WATCH_EMPTY]
        assert len(new) == 3
        e.write(40)
        e.poll()
    finally:
        e.close()


def test_whole_call_errors():
    e = Env()
    try:
        e.write(10)
        p = e.d.p
        f = p._f("watch_batch")
        blob = p.encode_watches([(NS1, e.revs[0]), (b"/", e.revs[0] - 1)])
        wids, sts, tot = (C.c_longlong * 2)(), (C.c_int * 2)(), C.c_ulonglong()

        def call(n, length, flags):
            return f(C.c_void_p(p.h), blob, C.c_size_t(length), C.c_size_t(n),
                     C.c_int(flags), wids, sts, C.byref(tot))

        first = p.watch(b"/")[1]
        assert call(2, len(blob), 1) == INVALID_ARG
        assert call(2, len(blob) - 1, 0) == INVALID_ARG   # prefix bytes run out
        assert call(2, 12 + len(NS1) + 11, 0) == INVALID_ARG   # header runs out
        assert call(0, 0, 0) == OK and tot.value == 0
        assert perf(p)["wreg_launches"] == 0
        assert call(2, len(blob), 0) == OK
        assert list(sts) == [OK, WATCH_LOW] and list(wids) == [first + 1, -1]
        assert p.watch(b"/")[1] == first + 2           # nothing else was registered
    finally:
        e.close()
