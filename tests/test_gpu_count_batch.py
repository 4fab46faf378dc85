"""GPU tests for kb_count_batch: n Counts in one call, every range cut into
row tiles that k_count_plan / k_count_tiles count across the chip (DESIGN.md
§3.8).

Reference for every entry: at rev == 0 the ORACLE's count(start, end) (through
parity.Dual.count, which also holds kb_count to it), at rev != 0 the length of
the oracle's unbounded list(start, end, rev). The whole expected reply (u32 n;
n x {i32 status; i32 0; u64 header_rev; u64 count}) is serialized in Python
and compared with the reply bytes as a whole. Every device case also asserts
from kb_perf_json that the kernels served every valid query, that a launch
happened, that k_range_scan2 stayed idle (scan_launches unchanged) and that
the tiles counted fit the rows covered, so a fallback to kb_count's one-block
scan cannot pass.
"""
import ctypes as C
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import benchwire as bw
import parity
import test_gpu_bench_records as tbr
from kbclient import BADKEY, COMPACTED, ENOBUF, INVALID_ARG, KEYTOOLONG, OK

pytestmark = pytest.mark.gpu

parity.small_env()

DEFAULT_TILE = 4096
COUNTERS = ("count_batch_calls", "count_batch_q", "count_batch_launches",
            "count_batch_tiles", "count_batch_rows", "scan_launches")


def v(tag, n=24):
    return ((b"%07d-" % tag) * (n // 8 + 1))[:n]


def expected_reply(entries):
    """entries = [(status, header_rev, count)] -> the reply bytes owed."""
    return struct.pack("<I", len(entries)) + b"".join(
        struct.pack("<iiQQ", st, 0, hr, c) for st, hr, c in entries)


def bound_status(b):
    """kb_count's validation of one bound (include/kb_slab.h: at most 4096
    bytes, no byte <= 0x24 except trailing 0x00). The oracle validates
    nothing, so for a bad bound kb_count itself is the reference."""
    if len(b) > 4096:
        return KEYTOOLONG
    return BADKEY if any(c <= 0x24 for c in b.rstrip(b"\x00")) else OK


def oracle_entry(d, q, cache=None):
    """What the issue's comparison rule owes query q = (start, end, rev,
    limit): count() at rev 0, len(list().kvs) at a named revision; for a bound
    kb_count rejects, kb_count's status and count 0."""
    s, e, rev, _limit = q
    hdr = d.o.current_rev()
    bad = bound_status(s) or bound_status(e)
    if bad:
        assert d.p.count(s, e) == (bad, hdr, 0)
        return (bad, hdr, 0)
    if rev == 0:
        rc, hr, c = d.count(s, e)          # oracle == kb_count, asserted
        assert hr == hdr
        return (rc, hdr, c if rc == OK else 0)
    key = (s, e, rev)
    if cache is not None and key in cache:
        return (OK, hdr, cache[key])
    lo = d.o.list(s, e, rev, 0)
    if lo.status != OK:
        return (lo.status, hdr, 0)
    if cache is not None:
        cache[key] = len(lo.kvs)
    return (OK, hdr, len(lo.kvs))


def check_batch(d, qs, tile=DEFAULT_TILE, want=None, cache=None, store=None,
                pending_scans=0, served=None):
    """One kb_count_batch of qs on the product against the oracle (or `want`,
    entries computed by the caller). pending_scans = range batches of a
    pipelined kb_bench_step the call collects first (their scan is accounted
    when they are collected); served = queries the kernels owe an answer,
    where that is not every KB_OK entry. -> (entries, counter deltas)."""
    p = store or d.p
    exp = want if want is not None else [oracle_entry(d, q, cache) for q in qs]
    nvalid = sum(st == OK for st, _, _ in exp) if served is None else served
    before = bw.perf(p)
    rc, res, raw = p.count_batch(qs)
    after = bw.perf(p)
    assert rc == OK, (rc, bw._err(p))
    want_raw = expected_reply(exp)
    if raw != want_raw:                      # say where, then fail on the whole
        for i, (a, b) in enumerate(zip(res, exp)):
            assert a == b, (i, qs[i][0][-30:], qs[i][1][-30:], qs[i][2], a, b)
    assert raw == want_raw
    assert res == exp
    delta = {k: after[k] - before[k] for k in COUNTERS}
    assert delta["count_batch_calls"] == 1, delta
    assert delta["count_batch_q"] == nvalid, (delta, nvalid)
    assert delta["scan_launches"] == pending_scans, delta   # k_range_scan2 idle
    rows, tiles = delta["count_batch_rows"], delta["count_batch_tiles"]
    if nvalid:
        assert delta["count_batch_launches"] >= 1, delta
    assert -(-rows // tile) <= tiles <= rows // tile + 2 * nvalid, (delta, nvalid)
    return exp, delta


def raw_call(store, qs, flags, cap, slack=64):
    """kb_count_batch with an exact cap and a canary behind it.
    -> (rc, out_len, total_count, bytes [0, cap), canary intact?)."""
    qbuf = store.encode_queries(qs)
    buf = C.create_string_buffer(b"\xc3" * (cap + slack), cap + slack)
    out_len = C.c_size_t(0)
    total = C.c_ulonglong(0)
    rc = store._f("count_batch")(C.c_void_p(store.h), qbuf, C.c_size_t(len(qs)),
                                 C.c_int(flags), buf, C.c_size_t(cap),
                                 C.byref(out_len), C.byref(total))
    mem = C.string_at(buf, cap + slack)
    return rc, out_len.value, total.value, mem[:cap], mem[cap:] == b"\xc3" * slack


@pytest.fixture(scope="module")
def world():
    """The bench-records fixture store: ~3000 rows over base and delta, keys
    with 1..5 versions, tombstones, recreated keys, 96/97/300-byte keys."""
    d = bw.open_dual()
    try:
        info = tbr.build(d)
        info["qs"] = tbr.make_queries(info)
        yield d, info
    finally:
        d.close()


# ---- 1. seeded mixed workload ------------------------------------------------
def test_seeded_mixed_workload():
    rng = random.Random(31)
    nss = [b"/registry/cm/ns-%d" % i for i in range(4)]
    keys = [ns + b"/k-%03d" % i for ns in nss for i in range(40)]
    d = bw.open_dual(KB_FLUSH_ROWS=512)
    try:
        live, revs = {}, []

        def op(n_op):
            k = keys[rng.randrange(len(keys))]
            if k not in live:
                r = d.create(k, v(n_op))
                if r.succeeded:
                    live[k] = r.header_revision
            elif rng.random() < 0.3:
                if d.delete(k, live[k]).succeeded:
                    del live[k]
            else:
                r = d.update(k, v(n_op), live[k])
                if r.succeeded:
                    live[k] = r.header_revision
            revs.append(d.p.current_rev())

        for n_op in range(600):
            op(n_op)
            if n_op % 40 == 39:
                d.count(nss[0] + b"/", nss[0] + b"0")    # device state current
        n_op = 600
        while True:
            d.count(nss[0] + b"/", nss[0] + b"0")
            p = bw.perf(d.p)
            if p["delta_rows"] > 0:
                break
            op(n_op)                                     # land rows in the delta
            n_op += 1
        assert p["base_rows"] > 0 and p["delta_rows"] > 0, p   # base AND delta
        ranges = []
        for ns in nss:
            ranges.append((ns + b"/", ns + b"0"))
            for _ in range(6):
                a = rng.randrange(39)
                b = rng.randrange(a + 1, 41)
                ranges.append((ns + b"/k-%03d" % a, ns + b"/k-%03d" % b))
        ranges.append((b"/registry/cm/", b"/registry/cm0"))
        cache = {}
        qs = [(s, e, r, 0) for r in [0] + revs[::10] for s, e in ranges]
        exp, delta = check_batch(d, qs, cache=cache)
        assert len(qs) > 1024 and delta["count_batch_launches"] >= 2  # sub-batches
        counts = [c for _, _, c in exp]
        assert max(counts) > 50 and counts.count(0) > 0
        assert len({c for c in counts}) > 20
        d.diff_dump()
    finally:
        d.close()


# ---- 2. tile edges -----------------------------------------------------------
def test_tile_edges():
    T = 64
    d = bw.open_dual(KB_COUNT_TILE=T, KB_FLUSH_ROWS=100000)
    try:
        keys = [b"/registry/te/obj-%04d" % i for i in range(300)]
        rev, hist = {}, []

        def txn(ops):
            out = bw.dual_txn(d, ops)
            assert all(out)
            for (k, _p, _v), r in zip(ops, out):
                rev[k] = r
            hist.extend(out)

        txn([(k, 0, v(i)) for i, k in enumerate(keys)])
        for gen, (mod, rem) in enumerate(((2, 0), (3, 1), (5, 2))):   # 1..4 versions
            txn([(k, rev[k], v(1000 * gen + i)) for i, k in enumerate(keys)
                 if i % mod == rem])
        dead = [k for i, k in enumerate(keys) if i % 11 == 4]
        outd = bw.dual_del(d, [(k, rev[k]) for k in dead])
        assert all(outd)
        hist.extend(outd)
        bw.flush(d.p)                                     # one run, rows in key order
        p = bw.perf(d.p)
        assert p["delta_rows"] == 0 and p["base_rows"] > 900, p
        end = b"/registry/te0"
        # every alignment of the first tile: the start bound slides over 130
        # consecutive keys (2..5 rows each, so the row offset passes every
        # residue mod 64 more than once)
        some = [0] + hist[5::61]
        qs = [(keys[j], end, some[(j + t) % len(some)], 0)
              for j in range(130) for t in range(3)]
        cache = {}
        exp, delta = check_batch(d, qs, tile=T, cache=cache)
        assert delta["count_batch_tiles"] > 2 * len(qs), delta
        assert len({c for _, _, c in exp}) > 100
        # every revision of the history over the whole range: for each key
        # whose rows straddle a tile edge, reads fall before, between and
        # after its revisions, so the last row of every tile meets both
        # outcomes of its look at the next tile's first row
        cur = d.p.current_rev()
        qs = [(keys[0], end, r, 0) for r in range(hist[0] - 1, cur + 2)]
        assert len(qs) > 600
        exp, delta = check_batch(d, qs, tile=T, cache=cache)
        assert delta["count_batch_tiles"] > 2 * len(qs), delta
        counts = [c for _, _, c in exp]
        assert counts[0] == 0 and max(counts) == 300
        assert counts[-1] == 300 - len(dead)
    finally:
        d.close()


# ---- 3. shadow suppression ---------------------------------------------------
def test_shadow_suppression_and_single_run_stores():
    T = 64
    ns = b"/registry/sh"
    d = bw.open_dual(KB_COUNT_TILE=T, KB_FLUSH_ROWS=100000)
    try:
        keys = [ns + b"/obj-%03d" % i for i in range(90)]
        ranges = [(ns + b"/", ns + b"0"), (keys[10], keys[70]),
                  (keys[3] + b"-", keys[44] + b"-"), (keys[50], keys[51])]
        rev1 = {k: d.create(k, v(i)).header_revision for i, k in enumerate(keys)}
        r_lo, r_mid = min(rev1.values()), rev1[keys[45]]
        revs1 = [0, r_lo - 1, r_lo, r_mid, r_mid + 1, max(rev1.values())]
        d.count(*ranges[0])                                # device state current
        p = bw.perf(d.p)
        assert p["base_rows"] == 0 and p["delta_rows"] > 0, p        # all delta
        qs1 = [(s, e, r, 0) for r in revs1 for s, e in ranges]
        exp, _ = check_batch(d, qs1, tile=T)
        assert exp[0][2] == 90
        bw.flush(d.p)
        p = bw.perf(d.p)
        assert p["base_rows"] > 0 and p["delta_rows"] == 0, p        # all base
        assert check_batch(d, qs1, tile=T)[0] == exp
        # updates and deletes left in the delta over the folded base rows
        drevs = []
        for i, k in enumerate(keys):
            if i % 4 == 1:
                r = d.update(k, v(500 + i), rev1[k])
                assert r.succeeded
                drevs.append(r.header_revision)
            elif i % 9 == 2:
                r = d.delete(k, rev1[k])
                assert r.succeeded
                drevs.append(r.header_revision)
        d.count(*ranges[0])
        p = bw.perf(d.p)
        assert p["base_rows"] > 0 and p["delta_rows"] > 0, p
        around = sorted({r + o for r in drevs for o in (-1, 0, 1)} | {0})
        qs2 = [(s, e, r, 0) for r in around for s, e in ranges] + qs1
        exp2, delta = check_batch(d, qs2, tile=T)
        by_q = dict(zip(qs2, exp2))
        ndel = sum(1 for i in range(90) if i % 4 != 1 and i % 9 == 2)
        assert by_q[ranges[0] + (0, 0)][2] == 90 - ndel
        assert by_q[ranges[0] + (drevs[0] - 1, 0)][2] == 90   # before the delta
        assert by_q[ranges[0] + (max(rev1.values()), 0)][2] == 90
        bw.flush(d.p)                                      # the same after the fold
        assert check_batch(d, qs2, tile=T)[0] == exp2
    finally:
        d.close()


# ---- 4. bounds ---------------------------------------------------------------
def test_bounds_long_keys(world):
    d, info = world
    p96, long_ = tbr.P96, tbr.LONG
    h = info["hist"]
    ranges = [(p96, p96 + b"c"), (long_[1], long_[4]), (long_[2], long_[2] + b"0"),
              (tbr.NS[3] + b"/long-", long_[0] + b"0"),
              (p96 + b"a" * 150, p96 + b"b" * 250), (long_[1], tbr.NS[3] + b"0")]
    assert max(len(e) for _, e in ranges) > 300 and min(len(s) for s, _ in ranges[:3]) >= 96
    qs = [(s, e, r, 0) for r in (0, h[0], h[2]) for s, e in ranges]
    exp, _ = check_batch(d, qs)
    assert max(c for _, _, c in exp[:3]) >= 2             # long keys were counted
    assert max(c for _, _, c in exp) > 100


def test_bounds_deleted_empty_inverted():
    d = bw.open_dual(KB_FLUSH_ROWS=100000)
    try:
        whole = (b"/registry/", b"/registry0")
        odd = [whole, (b"/registry/b", b"/registry/a"), (b"/registry/a", b"/registry/a"),
               (b"/registry/a", b""), (b"", b""), (b"", b"/registry0")]
        # empty store
        exp, delta = check_batch(d, [(s, e, 0, 0) for s, e in odd])
        assert [c for _, _, c in exp] == [0] * len(odd)
        assert delta["count_batch_rows"] == 0 and delta["count_batch_tiles"] == 0
        gone = [b"/registry/gone/k-%02d" % i for i in range(9)]
        kept = [b"/registry/kept/k-%02d" % i for i in range(5)]
        revs = {k: d.create(k, v(i)).header_revision for i, k in enumerate(gone + kept)}
        for k in gone:
            assert d.delete(k, revs[k]).succeeded
        cur = d.p.current_rev()
        dead_rng = (b"/registry/gone/", b"/registry/gone0")
        qs = [dead_rng + (0, 0), dead_rng + (cur, 0), whole + (0, 0)] + \
             [(s, e, 0, 0) for s, e in odd]
        exp, delta = check_batch(d, qs)
        assert exp[0][2] == 0 and exp[1][2] == 0 and exp[2][2] == 5
        assert delta["count_batch_rows"] > 0
        # inverted and empty bounds at a named revision: validation as Count's
        # (not List's KB_EINVALID), nothing to count
        want = [(OK, cur, 0)] * 4
        check_batch(d, [(s, e, cur, 0) for s, e in odd[1:5]], want=want)
        # after compaction only the revision rows of the deleted keys remain
        assert d.compact(cur)[0] == OK
        assert not any(ik[4:].startswith(b"/registry/gone/") and
                       int.from_bytes(ik[-8:], "big") for ik, _ in d.o.dump())
        bw.flush(d.p)
        exp, delta = check_batch(d, [dead_rng + (0, 0), dead_rng + (cur, 0),
                                     whole + (0, 0)])
        assert [c for _, _, c in exp] == [0, 0, 5]
    finally:
        d.close()


# ---- 5. statuses inside one batch ----------------------------------------------
def test_statuses_inside_one_batch(world):
    d, info = world
    ns = tbr.NS[1]
    good = (ns + b"/", ns + b"0")
    h = info["hist"]
    long_bound = b"/registry/" + b"k" * 4200
    qs = [good + (0, 0), (b"/registry/\x01x", b"/registry0", 0, 0), good + (h[1], 0),
          (ns + b"/", long_bound, 0, 0), good + (h[0], 7),
          (ns + b"/", b"/registry/p\x20q", h[1], 0), good + (0, 3)]
    exp, _ = check_batch(d, qs)
    assert [st for st, _, _ in exp] == [OK, BADKEY, OK, KEYTOOLONG, OK, BADKEY, OK]
    assert exp[0][2] > 100 and exp[0] == exp[6] and exp[2][2] > 0 and exp[4][2] > 0
    assert all(c == 0 for st, _, c in exp if st != OK)


def test_compacted_and_compat_off():
    ns = b"/registry/cp"
    d = bw.open_dual(KB_FLUSH_ROWS=100000)
    try:
        keys = [ns + b"/k-%02d" % i for i in range(30)]
        rev = {k: d.create(k, v(i)).header_revision for i, k in enumerate(keys)}
        for i, k in enumerate(keys[::3]):
            rev[k] = d.update(k, v(100 + i), rev[k]).header_revision
        mid = rev[keys[20]]
        for k in keys[1::5]:
            assert d.delete(k, rev[k]).succeeded
        cur = d.p.current_rev()
        assert d.compact(mid)[0] == OK
        rng_ = (ns + b"/", ns + b"0")
        qs = [rng_ + (0, 0), rng_ + (mid - 1, 0), rng_ + (mid, 0), rng_ + (1, 0),
              (keys[3], keys[9], cur, 0), rng_ + (mid + 2, 0),
              (b"/registry/\x02", ns + b"0", mid - 1, 0)]
        exp, delta = check_batch(d, qs)
        assert [st for st, _, _ in exp] == [OK, COMPACTED, OK, COMPACTED, OK, OK, BADKEY]
        assert exp[0][2] == 30 - len(keys[1::5]) and exp[2][2] > 0
        assert delta["count_batch_q"] == 4
    finally:
        d.close()
    # enable_etcd_compatibility = 0: all zeros, whatever the bounds, no kernel
    import kubebrain_amd
    with bw.env():
        s = kubebrain_amd.open_store(etcd_compat=False)
    try:
        s.set_current_rev(1000)
        for i in range(5):
            assert s.create(b"/registry/x/k-%d" % i, b"v").succeeded
        cur = s.current_rev()
        qs = [(b"/registry/", b"/registry0", 0, 0), (b"/registry/\x01", b"/r", 0, 0),
              (b"/registry/", b"/registry0", cur - 1, 0), (b"/registry/", b"", 5, 0)]
        assert s.count(b"/registry/", b"/registry0") == (OK, cur, 0)
        _, delta = check_batch(None, qs, want=[(OK, cur, 0)] * 4, store=s,
                               served=0)
        assert delta["count_batch_launches"] == 0 and delta["count_batch_q"] == 0
    finally:
        s.close()


# ---- 6. call shape -------------------------------------------------------------
def test_call_shape():
    ns = b"/registry/cs"
    max_q = 8
    d = bw.open_dual(KB_MAX_Q=max_q)
    try:
        keys = [ns + b"/k-%02d" % i for i in range(25)]
        for i, k in enumerate(keys):
            d.create(k, v(i))
        # n = 0
        rc, ln, tot, out, ok = raw_call(d.p, [], 0, 4)
        assert (rc, ln, tot, out, ok) == (OK, 4, 0, b"\x00\x00\x00\x00", True)
        assert d.p.count_batch([]) == (OK, [], b"\x00\x00\x00\x00")
        check_batch(d, [])
        # n = 2 KB_MAX_Q + 3: three launches, entries in query order
        n = 2 * max_q + 3
        qs = [(keys[i], keys[i + 1 + i % 6], 0, 0) for i in range(n)]
        qs[4] = (b"/registry/\x03", keys[0], 0, 0)        # one bad query inside
        exp, delta = check_batch(d, qs)
        assert delta["count_batch_launches"] == 3 and delta["count_batch_q"] == n - 1
        assert [c for _, _, c in exp] == [0 if i == 4 else 1 + i % 6 for i in range(n)]
        _, delta = check_batch(d, qs[5:5 + max_q])
        assert delta["count_batch_launches"] == 1
        _, delta = check_batch(d, qs[5:5 + max_q + 1])    # a ninth valid query
        assert delta["count_batch_launches"] == 2
        # flags
        for flags in (1, 2, -1, 1 << 30):
            before = bw.perf(d.p)
            rc, ln, tot, out, ok = raw_call(d.p, qs[:3], flags, 256)
            assert (rc, ln, tot, ok) == (INVALID_ARG, 0, 0, True), flags
            assert out == b"\xc3" * 256
            after = bw.perf(d.p)
            assert after["count_batch_launches"] == before["count_batch_launches"]
        # ENOBUF at need - 1, nothing written; success at exactly need
        need = 4 + 24 * n
        want_raw = expected_reply(exp)
        for cap in (need - 1, 4, 3, 0):
            before = bw.perf(d.p)
            rc, ln, tot, out, ok = raw_call(d.p, qs, 0, cap)
            after = bw.perf(d.p)
            assert (rc, ln, tot, ok) == (ENOBUF, need, 0, True), cap
            assert out == b"\xc3" * cap
            assert after["count_batch_launches"] == before["count_batch_launches"]
        rc, ln, tot, out, ok = raw_call(d.p, qs, 0, need)
        assert (rc, ln, ok) == (OK, need, True) and out == want_raw
        assert tot == sum(c for _, _, c in exp)
    finally:
        d.close()


# ---- 7. agreement with kb_count ------------------------------------------------
def test_agrees_with_kb_count(world):
    d, info = world
    qs = [(s, e, 0, lim) for s, e, _r, lim in info["qs"]]
    qs += [(b"/registry/pods/", b"/registry/pods0", 0, 0), (b"/registry/", b"/registry0", 0, 9)]
    want = [d.p.count(s, e) for s, e, _r, _l in qs]         # kb_count itself
    assert all(rc == OK for rc, _, _ in want)
    exp, _ = check_batch(d, qs, want=want)
    assert exp == [oracle_entry(d, q) for q in qs]          # and the oracle
    assert max(c for _, _, c in exp) > 1000
    assert sum(c == 0 for _, _, c in exp) > 5


# ---- 8. interleaving -------------------------------------------------------------
def test_interleaved_with_range_batches(world):
    d, info = world
    rq = info["qs"]
    cur = d.p.current_rev()
    exp = bw.expected(d, rq, cur)
    winners = sum(min(len(e), q[3]) if q[3] else len(e) for q, e in zip(rq, exp))
    cq = [(s, e, r, 0) for s, e, r, _l in rq[:60]]
    cache = {}
    want = [oracle_entry(d, q, cache) for q in cq]
    # the last Range batch's records survive a kb_count_batch byte for byte
    for mode, src in ((0, 0), (1, 1)):
        assert bw.bench_range(d.p, rq, mode) == winners
        raw0 = bw.last_range_raw(d.p, src)
        assert len(raw0) > 4 + 32 * len(rq)
        check_batch(d, cq, want=want)
        assert bw.last_range_raw(d.p, src) == raw0
    bw.check_records(rq, exp, bw.last_range(d.p, 0))
    # a count batch while a pipelined step's range batch is in flight: the
    # batch is collected first and its records stay where they were
    tot, _ = bw.bench_step(d.p, rq, [], 4)               # stays in flight
    check_batch(d, cq, want=want, pending_scans=1)
    bw.sync(d.p)
    bw.check_records(rq, exp, bw.last_range(d.p, 0))
    tot, _ = bw.bench_step(d.p, rq, [], 4)
    assert tot == 0                                      # nothing pending before it
    tot2, _ = bw.bench_step(d.p, rq, [], 4)              # reports the step before
    assert tot2 == winners, (tot2, winners)
    check_batch(d, cq[:9], want=want[:9], pending_scans=1)
    bw.sync(d.p)
    bw.check_records(rq, exp, bw.last_range(d.p, 0))
    # next to kb_list_batch, kb_get_batch, kb_count and kb_list
    rc, res1, sec1 = d.p.list_batch(rq[:12])
    assert rc == OK
    check_batch(d, cq, want=want)
    rc, res2, sec2 = d.p.list_batch(rq[:12])
    assert rc == OK and sec2 == sec1
    for s, e, r, lim in rq[:4]:
        d.list(s, e, r, lim)
        d.count(s, e)
    check_batch(d, cq, want=want)
