"""GPU tests for kb_list_batch: n Range queries in one call, their sections
serialized on the device straight from the scan's winner rows (k_list_size /
k_list_emit).

Reference for every section: the ORACLE's List of the same query,
re-serialized in Python to the kb_list wire bytes (values blanked first for
keys_only). Parsed kvs, `more`, header_rev and the raw section bytes must all
be equal. Device-path cases also assert from kb_perf_json that the kernels
served every OK query (list_batch_q_dev), that none fell back to the host path
(list_batch_q_host == 0) and that the gather kernels never ran
(gather_launches unchanged), so a silent fallback cannot pass.
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
from kbclient import (BADKEY, COMPACTED, ENOBUF, INVALID_ARG, KEYTOOLONG, OK,
                      Kv)
from test_list_plan import model as plan_model

pytestmark = pytest.mark.gpu

parity.small_env()

VLENS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 511, 512, 513]
COUNTERS = ("list_batch_calls", "list_batch_q_dev", "list_batch_q_host",
            "list_batch_kvs", "list_batch_bytes", "list_emit_launches",
            "gather_launches", "scan_launches")


def ser(kvs):
    out = [struct.pack("<I", len(kvs))]
    for kv in kvs:
        out.append(struct.pack("<QI", kv.revision, len(kv.key)))
        out.append(kv.key)
        out.append(struct.pack("<I", len(kv.value)))
        out.append(kv.value)
    return b"".join(out)


def fmt(kvs):
    return [(k.key, k.value, k.revision) for k in kvs]


def check_batch(d, qs, keys_only=False, path=None, product_only=()):
    """One kb_list_batch of qs on the product against the oracle's List of
    each query. product_only = indices whose status the oracle cannot produce
    (bound validation is the product's): those are compared with kb_list.
    path "dev": every OK query must have been served by the kernels.
    -> (results, raw sections, counter deltas, oracle responses)."""
    exp = [None if i in product_only else d.o.list(*q) for i, q in enumerate(qs)]
    before = bw.perf(d.p)
    rc, res, raw = d.p.list_batch(qs, keys_only)
    after = bw.perf(d.p)
    assert rc == OK, (rc, bw._err(d.p))
    assert len(res) == len(raw) == len(qs)
    cur = d.p.current_rev()
    nok = nkv = 0
    for i, (q, lo) in enumerate(zip(qs, exp)):
        st, rp = res[i]
        assert rp.header_revision == cur, (i, rp.header_revision, cur)
        if lo is None:
            want = d.p.list(*q).status          # what kb_list gives
            assert want != OK and st == want, (i, q, st, want)
            assert raw[i] == b"" and not rp.kvs
            continue
        assert st == lo.status, (i, q, st, lo.status)
        if st != OK:
            assert raw[i] == b"" and not rp.kvs, i
            continue
        nok += 1
        assert lo.header_revision == cur
        kvs = [Kv(k.key, b"", k.revision) for k in lo.kvs] if keys_only else lo.kvs
        nkv += len(kvs)
        assert len(rp.kvs) == len(kvs), (i, q, len(rp.kvs), len(kvs))
        assert fmt(rp.kvs) == fmt(kvs), (i, q)
        assert rp.more == lo.more, (i, q, rp.more, lo.more)
        assert raw[i] == ser(kvs), (i, q)
    delta = {k: after[k] - before[k] for k in COUNTERS}
    assert delta["list_batch_calls"] == 1
    assert delta["list_batch_kvs"] == nkv
    assert delta["list_batch_q_dev"] + delta["list_batch_q_host"] == nok
    if path == "dev":
        assert delta["list_batch_q_dev"] == nok, delta
        assert delta["list_batch_q_host"] == 0, delta
        assert delta["gather_launches"] == 0, delta
        if nkv:
            assert delta["list_emit_launches"] >= 1 and delta["list_batch_bytes"] > 0
    return res, raw, delta, exp


def raw_call(store, qs, flags, cap, slack=64):
    """kb_list_batch with an exact cap and a canary behind it.
    -> (rc, out_len, total_kvs, bytes [0, cap), canary intact?)."""
    qbuf = store.encode_queries(qs)
    buf = C.create_string_buffer(b"\xc3" * (cap + slack), cap + slack)
    out_len = C.c_size_t(0)
    total = C.c_ulonglong(0)
    rc = store._f("list_batch")(C.c_void_p(store.h), qbuf, C.c_size_t(len(qs)),
                                C.c_int(flags), buf, C.c_size_t(cap),
                                C.byref(out_len), C.byref(total))
    mem = C.string_at(buf, cap + slack)
    return rc, out_len.value, total.value, mem[:cap], mem[cap:] == b"\xc3" * slack


def skey(ns, i, total):
    """A key of exactly `total` bytes, ordered by i."""
    k = ns + b"/%03d-" % i
    assert len(k) <= total
    return k + b"k" * (total - len(k))


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


# ---- 1. alignment sweep ------------------------------------------------------
def test_alignment_sweep():
    ns = b"/registry/al"
    klens = list(range(20, 37)) + [95, 96, 97, 112, 113, 300]
    d = bw.open_dual()
    try:
        keys = []
        for i in range(81):
            k = skey(ns, i, klens[i % len(klens)])
            keys.append(k)
            d.create(k, bytes([0x30 + i % 64]) * VLENS[i % len(VLENS)])
        count = len(keys)
        lo, hi = ns + b"/", ns + b"0"
        qs = [(lo, hi, 0, lim) for lim in (1, 2, count - 1, count, count + 1, 0)]
        qs += [(keys[a], keys[b], 0, lim)
               for a, b, lim in ((3, 40, 0), (17, 18, 0), (20, 80, 9), (5, 6, 1))]
        res, raw, _delta, exp = check_batch(d, qs, path="dev")
        assert [len(r.kvs) for _, r in res[:6]] == \
            [1, 2, count - 1, count, count, count]
        assert [r.more for _, r in res[:6]] == [True, True, True, False, False, False]
        # destination residues, from the expected bytes: the arena is laid out
        # like the reply from the first section on (one round), 16 B aligned
        base = 4 + 24 * len(qs)
        off = base
        rec_res, key_res, val_res = set(), set(), set()
        for lo_ in exp:
            off += 4
            for kv in lo_.kvs:
                a = off - base
                rec_res.add(a % 16)
                key_res.add((a + 12) % 16)
                val_res.add((a + 16 + len(kv.key)) % 16)
                off += 16 + len(kv.key) + len(kv.value)
        assert rec_res == key_res == val_res == set(range(16))
        got_klens = {len(k.key) for _, r in res for k in r.kvs}
        assert set(klens) <= got_klens
        assert set(VLENS) <= {len(k.value) for _, r in res for k in r.kvs}
    finally:
        d.close()


# ---- 2. MVCC content ---------------------------------------------------------
def test_mvcc_content(world):
    d, info = world
    qs = info["qs"]
    p = bw.perf(d.p)
    assert p["base_rows"] > 0 and p["delta_rows"] > 0, p   # base AND delta
    res, raw, _delta, exp = check_batch(d, qs, path="dev")
    assert {q[3] for q in qs} == {0, 1, 7, 500}
    assert len({q[2] for q in qs}) == 5                     # old revisions too
    # empty ranges: section = u32 0
    empties = [i for i, lo in enumerate(exp) if not lo.kvs]
    assert len(empties) >= 10
    assert all(raw[i] == b"\x00\x00\x00\x00" for i in empties)
    assert sum(1 for _, r in res if r.more) >= 10
    # tombstone winners are dropped at the latest revision, present before
    dead = set(info["dead"])
    latest = {k.key for q, (_s, r) in zip(qs, res) if q[2] == 0 for k in r.kvs}
    old = {k.key for q, (_s, r) in zip(qs, res) if q[2] == info["hist"][0]
           for k in r.kvs}
    recreated = {k for i, k in enumerate(info["dead"]) if i % 3 == 0}
    assert not (latest & (dead - recreated))
    assert old & (dead - recreated)
    # several revisions per key were in play
    assert len({k.revision for _, r in res for k in r.kvs}) > 100
    assert {len(k.key) for _, r in res for k in r.kvs} >= {96, 97, 300}


# ---- 3. per-query statuses ---------------------------------------------------
def test_statuses_in_one_batch():
    ns = b"/registry/st"
    d = bw.open_dual()
    try:
        keys = [skey(ns, i, 24 + i % 5) for i in range(30)]
        rev = {}
        for i, k in enumerate(keys):
            rev[k] = d.create(k, b"v" * (i * 7 % 40)).header_revision
        mid = d.p.current_rev()
        for i, k in enumerate(keys[::3]):
            assert d.update(k, b"w" * (i + 1), rev[k]).succeeded
        assert d.compact(mid)[0] == OK
        good = [(ns + b"/", ns + b"0", 0, 0), (keys[2], keys[20], 0, 5),
                (keys[4], keys[9], mid, 0), (ns + b"/", ns + b"0", 0, 3)]
        qs = [good[0],
              (ns + b"/", b"", 0, 0),                      # empty end
              good[1],
              (keys[9], keys[4], 0, 0),                    # start >= end
              (keys[9], keys[9], 0, 0),
              (ns + b"/a\x01b", ns + b"0", 0, 0),          # key byte <= 0x24
              good[2],
              (ns + b"/", ns + b"/" + b"x" * 4097, 0, 0),  # bound over 4096 B
              (ns + b"/", ns + b"0", mid - 1, 0),          # below the compact rev
              good[3]]
        res, raw, delta, _exp = check_batch(d, qs, path="dev", product_only={5, 7})
        assert [st for st, _ in res] == [OK, INVALID_ARG, OK, INVALID_ARG,
                                         INVALID_ARG, BADKEY, OK, KEYTOOLONG,
                                         COMPACTED, OK]
        assert delta["list_batch_q_dev"] == 4
        # kb_list agrees on every status, and on the good ones' bytes
        for q, (st, r) in zip(qs, res):
            one = d.p.list(*q)
            assert one.status == st
            if st == OK:
                assert fmt(one.kvs) == fmt(r.kvs) and one.more == r.more
        # an all-error batch is a directory alone
        rc, n, tot, out, ok = raw_call(d.p, [qs[1], qs[3]], 0, 4 + 48)
        assert (rc, n, tot, ok) == (OK, 52, 0, True)
        assert struct.unpack_from("<I", out, 0) == (2,)
        assert struct.unpack_from("<iiQQ", out, 4)[::3] == (INVALID_ARG, 0)
    finally:
        d.close()


# ---- 4. ENOBUF ---------------------------------------------------------------
def test_enobuf(world):
    d, info = world
    qs = info["qs"][:40]
    n = len(qs)
    rc, required, total, fresh, ok = raw_call(d.p, qs, 0, 8 << 20)
    assert rc == OK and ok and total > 0
    fresh = fresh[:required]
    assert required > 4 + 24 * n
    for cap in (required - 1, 4 + 24 * n - 1, 3):
        before = bw.perf(d.p)
        rc, out_len, _tot, _out, ok = raw_call(d.p, qs, 0, cap)
        after = bw.perf(d.p)
        assert rc == ENOBUF, (cap, rc)
        assert out_len == required, (cap, out_len, required)
        assert ok, cap                                       # canary after cap
        assert after["list_emit_launches"] == before["list_emit_launches"]
        assert after["list_batch_bytes"] == before["list_batch_bytes"]
        assert after["gather_launches"] == before["gather_launches"]
        rc, out_len, tot2, out, ok = raw_call(d.p, qs, 0, required)
        assert (rc, out_len, tot2, ok) == (OK, required, total, True)
        assert out == fresh
    # and the bytes are the oracle's
    check_batch(d, qs, path="dev")


# ---- 5. fallback -------------------------------------------------------------
def test_host_fallback_small_winner_table():
    big, small = b"/registry/fb/big", b"/registry/fb/sml"
    d = bw.open_dual(KB_MAX_CAP=64)
    try:
        bk = [skey(big, i, 22 + i % 9) for i in range(150)]
        sk = [skey(small, i, 95 + i % 4) for i in range(30)]
        for i, k in enumerate(bk + sk):
            d.create(k, bytes([0x41 + i % 26]) * VLENS[i % len(VLENS)])
        qs = [(big + b"/", big + b"0", 0, 0),        # 150 winners > 64: host
              (small + b"/", small + b"0", 0, 0),    # 30 winners: device
              (big + b"/", big + b"0", 0, 100),      # limit+1 > 64: host
              (big + b"/", big + b"0", 0, 63),       # limit+1 == 64: device
              (big + b"/", big + b"0", 0, 64),       # limit+1 == 65: host
              (small + b"/", small + b"0", 0, 10),   # device
              (bk[10], bk[74], 0, 0),                # exactly 64 winners: host
              (bk[10], bk[73], 0, 0),                # 63 winners: device
              (bk[0], bk[5], 0, 1000),               # limit+1 > 64: host
              (big + b"0", small + b"/", 0, 0)]      # nothing in between: device
        res, raw, delta, exp = check_batch(d, qs)
        assert [len(lo.kvs) for lo in exp] == [150, 30, 100, 63, 64, 10, 64, 63, 5, 0]
        assert [lo.more for lo in exp] == [False, False, True, True, True, True,
                                          False, False, False, False]
        assert delta["list_batch_q_host"] == 5, delta
        assert delta["list_batch_q_dev"] == 5, delta
        # keys_only takes the same paths with the same bytes minus values
        _res, _raw, delta, _exp = check_batch(d, qs, keys_only=True)
        assert (delta["list_batch_q_host"], delta["list_batch_q_dev"]) == (5, 5)
    finally:
        d.close()


# ---- 6. sub-batches and rounds -----------------------------------------------
def test_sub_batches_and_rounds():
    ns = b"/registry/sb"
    arena = 16384
    d = bw.open_dual(KB_MAX_Q=8, KB_ARENA_BYTES=arena)
    try:
        keys = [skey(ns, i, 21 + i % 7) for i in range(64)]
        for i, k in enumerate(keys):
            d.create(k, bytes([0x61 + i % 26]) * (290 + i % 23))
        qs = [(keys[2 * i], keys[2 * i + 11], 0, 0 if i % 3 else 9)
              for i in range(20)]
        qs[7] = (keys[5], keys[5], 0, 0)              # an error between them
        qs[13] = (keys[40] + b"-", keys[40] + b"-z", 0, 0)   # an empty one
        res, raw, delta, exp = check_batch(d, qs, path="dev")
        # 19 device queries in sub-batches of 8, 8 and 3; every section fits
        # the arena, the sections of a full sub-batch do not: 2 + 2 + 1 rounds
        # at the least
        st = [lo.status for lo in exp]
        lens = [len(r) for r in raw]
        assert max(lens) <= arena
        group, g, c = [], 0, 0
        for s in st:
            if s == OK:
                if c == 8:
                    g, c = g + 1, 0
                c += 1
            group.append(g if s == OK else -1)
        m = plan_model(st, [-1] * 20, [max(ln - 4, 0) for ln in lens], arena, group)
        assert m["required"] == 4 + 24 * 20 + sum(lens)
        rounds_with_records = {m["round"][i] for i in range(20)
                               if st[i] == OK and exp[i].kvs}
        assert sum(lens[:8]) > arena and len(m["rounds"]) >= 5
        assert delta["list_emit_launches"] == len(rounds_with_records) >= 5, delta
        # n == 0 and n == 1
        rc, n, tot, out, ok = raw_call(d.p, [], 0, 4)
        assert (rc, n, tot, out, ok) == (OK, 4, 0, b"\x00\x00\x00\x00", True)
        rc, n, tot, out, ok = raw_call(d.p, [], 0, 3)
        assert (rc, n, ok) == (ENOBUF, 4, True)
        assert d.p.list_batch([]) == (OK, [], [])
        check_batch(d, qs[:1], path="dev")
        check_batch(d, [qs[13]], path="dev")
    finally:
        d.close()


# ---- 7. keys_only and flags --------------------------------------------------
def test_keys_only_and_bad_flags(world):
    d, info = world
    qs = info["qs"][::2]
    res, raw, _delta, _exp = check_batch(d, qs, keys_only=True, path="dev")
    assert all(k.value == b"" for _, r in res for k in r.kvs)
    assert sum(len(r.kvs) for _, r in res) > 500
    full = d.p.list_batch(qs)[2]
    assert sum(map(len, raw)) < sum(map(len, full))
    for flags in (2, 3, 4, 1 << 30, -1):
        before = bw.perf(d.p)
        rc, n, tot, _out, ok = raw_call(d.p, qs[:3], flags, 1 << 16)
        assert (rc, n, tot, ok) == (INVALID_ARG, 0, 0, True), flags
        assert bw.perf(d.p)["scan_launches"] == before["scan_launches"]


# ---- 8. interleaving with the pipelined bench step ---------------------------
def test_interleaved_with_pipelined_bench_step(world):
    d, info = world
    qs = info["qs"]
    cur = d.p.current_rev()
    exp = bw.expected(d, qs, cur)
    winners = sum(min(len(e), q[3]) if q[3] else len(e) for q, e in zip(qs, exp))
    tot, _ = bw.bench_step(d.p, qs, [], 4)         # stays in flight

    def over_pending(sub):
        # the call collects the in-flight bench batch first: that batch's own
        # gather launch is the one counted here, the list path adds none
        _res, _raw, delta, exp_ = check_batch(d, sub)
        assert delta["list_batch_q_host"] == 0, delta
        assert delta["list_batch_q_dev"] == sum(lo.status == OK for lo in exp_)
        assert delta["gather_launches"] == 1, delta

    over_pending(qs[10:70])
    # the arena now holds wire sections, not gathered records
    assert bw.last_range(d.p, 0) == []
    check_batch(d, qs[:10], path="dev")            # nothing pending: no gather
    tot, _ = bw.bench_step(d.p, qs, [], 4)
    assert tot == 0                                # nothing pending before it
    over_pending(qs[70:90])
    tot, _ = bw.bench_step(d.p, qs, [], 4)
    tot2, _ = bw.bench_step(d.p, qs, [], 4)        # reports the step before
    assert tot2 == winners, (tot2, winners)
    bw.sync(d.p)
    bw.check_records(qs, exp, bw.last_range(d.p, 0))
    assert bw.bench_range(d.p, qs, 0) == winners
    bw.check_records(qs, exp, bw.last_range(d.p, 0))


# ---- 9. seeded soak ----------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_soak(seed):
    rng = random.Random(seed)
    nss = [b"/registry/sk/ns-%d" % i for i in range(3)]
    keys = [skey(ns, i, 24 + (i * 5 + j) % 19) for j, ns in enumerate(nss)
            for i in range(40)]
    keys += [skey(nss[1], 900 + i, L) for i, L in enumerate((96, 97, 130, 300))]
    keys.sort()
    d = bw.open_dual()
    try:
        live, revs = {}, [d.p.current_rev()]
        seen_status = set()
        for op in range(1, 301):
            k = keys[rng.randrange(len(keys))]
            v = bytes([0x30 + op % 70]) * VLENS[rng.randrange(len(VLENS))]
            roll = rng.random()
            if k not in live:
                r = d.create(k, v)
                if r.succeeded:
                    live[k] = r.header_revision
            elif roll < 0.3:
                if d.delete(k, live[k]).succeeded:
                    del live[k]
            else:
                r = d.update(k, v, live[k])
                if r.succeeded:
                    live[k] = r.header_revision
            if op % 97 == 0:
                d.compact(revs[len(revs) // 2])
            if op % 50:
                continue
            revs.append(d.p.current_rev())
            qs = []
            for _ in range(30):
                a = rng.randrange(len(keys) - 1)
                b = min(len(keys) - 1, a + 1 + rng.randrange(45))
                s, e = keys[a], keys[b]
                if rng.random() < 0.3:
                    s += b"-"
                if rng.random() < 0.3:
                    e += b"-"
                rev = rng.choice([0, 0, revs[-1]] + revs)
                qs.append((s, e, rev, rng.choice([0, 0, 1, 2, 5, 17, 500])))
            ns = nss[rng.randrange(3)]
            qs.append((ns + b"/", ns + b"0", 0, 0))
            res, _raw, _delta, _exp = check_batch(d, qs, path="dev")
            seen_status |= {st for st, _ in res}
        assert {OK, COMPACTED} <= seen_status, seen_status
        d.diff_dump()
    finally:
        d.close()
