"""GPU tests for kb_get_batch: n point reads in one call, the reply's
directory and the packed value bytes written on the device (k_get_find /
k_get_plan / k_get_emit).

Reference for every entry: the ORACLE's get(key, rev). The whole expected
reply (u32 n; n x {i32 status; i32 has_kv; u64 header_rev; u64 mod_rev; u64
vlen}; then the values) is serialized in Python and compared with the reply
bytes as a whole. Device-path cases also assert from kb_perf_json that the
kernels served every query (get_batch_q_dev == n, get_batch_q_host == 0),
that a launch happened and that k_get2 stayed idle (get_launches unchanged),
so a silent fallback to kb_get's path or to the host cannot pass.
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
from kbclient import ENOBUF, INVALID_ARG, OK
from test_get_plan import model as plan_model

pytestmark = pytest.mark.gpu

parity.small_env()

VLENS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 511, 512, 513, 4095, 4096,
         4097, 8191, 8193, 16384, 16385, 20001]
KLENS = list(range(20, 37)) + [95, 96, 97, 300]
COUNTERS = ("get_batch_calls", "get_batch_q_dev", "get_batch_q_host",
            "get_batch_found", "get_batch_bytes", "get_batch_launches",
            "get_launches")


def skey(ns, i, total):
    """A key of exactly `total` bytes, ordered by i."""
    k = ns + b"/%03d-" % i
    assert len(k) <= total
    return k + b"k" * (total - len(k))


def blob(tag, n):
    """n value bytes that differ from offset to offset and from tag to tag."""
    return bytes((tag * 7 + j * 13 + (j >> 8)) % 251 + 1 for j in range(n))


def expected_reply(entries, no_values=False):
    """entries = [(rc, header_rev, Kv | None)] as the oracle's get returns
    them -> the reply bytes kb_get_batch owes."""
    head, vals = [struct.pack("<I", len(entries))], []
    for rc, hr, kv in entries:
        v = b"" if kv is None or no_values else kv.value
        head.append(struct.pack("<iiQQQ", rc, 1 if kv else 0, hr,
                                kv.revision if kv else 0, len(v)))
        vals.append(v)
    return b"".join(head + vals)


def check_batch(d, qs, no_values=False, path="dev", want=None):
    """One kb_get_batch of qs = [(key, rev)] on the product against the
    oracle's get of each query (or `want`, entries computed by the caller).
    -> (entries, reply bytes, counter deltas)."""
    exp = want if want is not None else [d.o.get(k, r) for k, r in qs]
    before = bw.perf(d.p)
    rc, res, raw = d.p.get_batch(qs, no_values)
    after = bw.perf(d.p)
    assert rc == OK, (rc, bw._err(d.p))
    want_raw = expected_reply(exp, no_values)
    if raw != want_raw:                      # say where, then fail on the whole
        n = len(qs)
        for i in range(n):
            a, b = raw[4 + 32 * i:36 + 32 * i], want_raw[4 + 32 * i:36 + 32 * i]
            assert a == b, (i, qs[i][0][:40], qs[i][1],
                            struct.unpack("<iiQQQ", a), struct.unpack("<iiQQQ", b))
        off = 4 + 32 * n
        for i, (_rc, _hr, kv) in enumerate(exp):
            ln = 0 if kv is None or no_values else len(kv.value)
            assert raw[off:off + ln] == want_raw[off:off + ln], \
                ("value bytes", i, qs[i][0][:40], qs[i][1], ln)
            off += ln
    assert raw == want_raw
    found = sum(kv is not None for _, _, kv in exp)
    assert [(st, hr, kv) for st, hr, kv in res] == \
        [(rc_, hr, None if kv is None else
          type(kv)(kv.key, b"" if no_values else kv.value, kv.revision))
         for rc_, hr, kv in exp]
    delta = {k: after[k] - before[k] for k in COUNTERS}
    assert delta["get_batch_calls"] == 1
    assert delta["get_batch_found"] == found
    assert delta["get_batch_q_dev"] + delta["get_batch_q_host"] == len(qs)
    assert delta["get_launches"] == 0, delta         # k_get2 stayed idle
    if path == "dev":
        assert delta["get_batch_q_host"] == 0, delta
        assert delta["get_batch_q_dev"] == len(qs), delta
        if qs:
            assert delta["get_batch_launches"] >= 1, delta
        nbytes = len(raw) - 4 - 32 * len(qs)
        assert delta["get_batch_bytes"] == nbytes, (delta, nbytes)
    return exp, raw, delta


def raw_call(store, qs, flags, cap, slack=64):
    """kb_get_batch with an exact cap and a canary behind it.
    -> (rc, out_len, total_found, bytes [0, cap), canary intact?)."""
    qbuf = store.encode_gets(qs)
    buf = C.create_string_buffer(b"\xc3" * (cap + slack), cap + slack)
    out_len = C.c_size_t(0)
    total = C.c_ulonglong(0)
    rc = store._f("get_batch")(C.c_void_p(store.h), qbuf, C.c_size_t(len(qs)),
                               C.c_int(flags), buf, C.c_size_t(cap),
                               C.byref(out_len), C.byref(total))
    mem = C.string_at(buf, cap + slack)
    return rc, out_len.value, total.value, mem[:cap], mem[cap:] == b"\xc3" * slack


def versions(d):
    """{user key: sorted object-row revisions} from the oracle's dump
    (internal key = 4-byte magic | user key | '$' | u64 BE revision; the
    revision-0 rows are the rev-index)."""
    out = {}
    for ik, _v in d.o.dump():
        rev = int.from_bytes(ik[-8:], "big")
        if rev:
            out.setdefault(ik[4:-9], []).append(rev)
    return {k: sorted(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def world():
    """The bench-records fixture store: ~3000 rows over base and delta, keys
    with 1..5 versions, tombstones, recreated keys, 96/97/300-byte keys."""
    d = bw.open_dual()
    try:
        info = tbr.build(d)
        info["qs"] = tbr.make_queries(info)
        info["vers"] = versions(d)
        yield d, info
    finally:
        d.close()


# ---- 1. alignment and chunk sweep --------------------------------------------
def test_alignment_and_chunk_sweep():
    ns = b"/registry/al"
    d = bw.open_dual()
    try:
        keys = []
        for i in range(3 * len(VLENS)):
            k = skey(ns, i, KLENS[i % len(KLENS)])
            keys.append((k, VLENS[i % len(VLENS)]))
            d.create(k, blob(i, VLENS[i % len(VLENS)]))
        small = {vl: k for k, vl in keys if 0 < vl < 16}
        bigs = [k for k, vl in keys if vl >= 32]
        vlen_of = dict(keys)
        # order: before the j-th big value, spacers of 1..15 bytes steer the
        # running offset to residue j mod 16; the rest of the keys follow
        order, cur = [], 0
        for j, k in enumerate(bigs):
            gap = (j - cur) % 16
            for sp in (15, 5, 4, 3, 2, 1):
                while gap >= sp:
                    order.append(small[sp])
                    gap -= sp
                    cur += sp
            order.append(k)
            cur += vlen_of[k]
        order += [k for k, _ in keys if k not in set(order)]
        qs = [(k, 0) for k in order]
        exp, raw, _delta = check_batch(d, qs, path="dev")
        # a condition on the inputs: destination residues of the values of 32
        # bytes and more, from the expected layout (the arena is laid out like
        # the reply's value span, its base 16-byte aligned)
        off, residues = 0, set()
        for _rc, _hr, kv in exp:
            assert kv is not None
            if len(kv.value) >= 32:
                residues.add(off % 16)
            off += len(kv.value)
        assert residues == set(range(16)), residues
        assert {len(kv.value) for _, _, kv in exp} == set(VLENS)
        assert {len(k) for k, _ in qs} == set(KLENS)
        assert len(qs) > len(keys)                  # keys repeat in the batch
    finally:
        d.close()


# ---- 2. MVCC semantics -------------------------------------------------------
def test_mvcc_semantics(world):
    d, info = world
    vers, cur = info["vers"], info["cur"]
    p = bw.perf(d.p)
    assert p["base_rows"] > 0 and p["delta_rows"] > 0, p     # base AND delta
    assert max(map(len, vers.values())) >= 5
    qs = []
    for k in info["keys"] + info["fat"]:
        revs = {0, cur + 10}
        for r in vers[k]:
            revs |= {r - 1, r, r + 1}                # first - 1 = before the key
        qs += [(k, r) for r in sorted(revs)]
    keys = sorted(info["keys"])
    p96 = tbr.P96
    absent = [b"/registry/a", b"/registry/zzz", keys[0][:-1], keys[-1] + b"0",
              keys[10] + b"-", keys[11][:-3], keys[500] + b"x", keys[500][:-1],
              p96[:95], p96 + b"c", p96 + b"a" * 203, p96 + b"a" * 205,
              p96 + b"b" * 2, p96 + b"ab"]
    assert not set(absent) & set(vers)
    qs += [(k, r) for k in absent for r in (0, info["hist"][1])]
    exp, _raw, delta = check_batch(d, qs, path="dev")
    assert len(qs) > 3 * int(os.environ.get("KB_MAX_Q", 1024))   # sub-batches
    assert delta["get_batch_launches"] >= 4
    n_abs = 2 * len(absent)
    assert all(kv is None for _, _, kv in exp[-n_abs:])
    # tombstone winners: not found at the delete's revision, found before
    dead = [k for i, k in enumerate(info["dead"]) if i % 3]     # not recreated
    by_q = dict(zip(qs, exp))
    for k in dead[:20]:
        t = vers[k][-1]
        assert by_q[(k, t)][2] is None and by_q[(k, 0)][2] is None
        assert by_q[(k, t - 1)][2] is not None
        assert by_q[(k, t)][1] == cur                # header = committed revision
    assert sum(kv is None for _, _, kv in exp) > 1000
    assert sum(kv is not None for _, _, kv in exp) > 3000
    assert {len(kv.key) for _, _, kv in exp if kv} >= {96, 97, 300}
    # keys kb_get does not validate either: whatever kb_get says
    odd = [(b"", 0), (b"/registry/\x01x", 0), (b"$", 0), (b"/registry/" + b"k" * 4200, 0)]
    want = [d.p.get(k, r) for k, r in odd]
    assert all(kv is None for _, _, kv in want)
    check_batch(d, odd, path="dev", want=want)


# ---- 3. runs -----------------------------------------------------------------
def test_runs_empty_delta_base_compacted():
    ns = b"/registry/rn"
    d = bw.open_dual(KB_FLUSH_ROWS=100000)
    try:
        keys = [skey(ns, i, 22 + i % 9) for i in range(40)] + \
               [skey(ns, 900, 96), skey(ns, 901, 97), skey(ns, 902, 300)]
        check_batch(d, [(k, 0) for k in keys[:5]], path="dev")      # empty store
        rev1 = {k: d.create(k, blob(i, 30 + 17 * i)).header_revision
                for i, k in enumerate(keys)}
        d.get(keys[0])                                # device state current
        p = bw.perf(d.p)
        assert p["base_rows"] == 0 and p["delta_rows"] > 0, p      # all delta
        every = [(k, r) for k in keys for r in (0, rev1[k], rev1[k] - 1)]
        check_batch(d, every, path="dev")
        bw.flush(d.p)                                 # fold: all base
        p = bw.perf(d.p)
        assert p["base_rows"] > 0 and p["delta_rows"] == 0, p
        check_batch(d, every, path="dev")
        # newest version in the delta over an older base version
        rev2 = {}
        for i, k in enumerate(keys[::2]):
            r = d.update(k, blob(i + 100, 500 + 33 * i), rev1[k])
            assert r.succeeded
            rev2[k] = r.header_revision
        gone = keys[1]
        assert d.delete(gone, rev1[gone]).succeeded
        d.get(keys[0])
        p = bw.perf(d.p)
        assert p["base_rows"] > 0 and p["delta_rows"] > 0, p
        both = every + [(k, r) for k in rev2 for r in (rev2[k], rev2[k] - 1)]
        exp, _raw, _delta = check_batch(d, both, path="dev")
        by_q = dict(zip(both, exp))
        k0 = keys[0]
        assert by_q[(k0, 0)][2].revision == rev2[k0]
        assert by_q[(k0, rev1[k0])][2].revision == rev1[k0]
        assert by_q[(gone, 0)][2] is None and by_q[(gone, rev1[gone])][2] is not None
        bw.flush(d.p)                                 # the same after the fold
        assert bw.perf(d.p)["delta_rows"] == 0
        check_batch(d, both, path="dev")
        mid = max(rev1.values()) + 3                  # among the updates' revisions
        assert d.compact(mid)[0] == OK
        check_batch(d, both + [(k, mid - 5) for k in keys], path="dev")
    finally:
        d.close()


# ---- 4. sub-batches ----------------------------------------------------------
def test_sub_batches():
    ns = b"/registry/sb"
    d = bw.open_dual(KB_MAX_Q=8)
    try:
        keys = [skey(ns, i, 21 + i % 7) for i in range(12)]
        for i, k in enumerate(keys):
            d.create(k, blob(i, 100 + 31 * i))
        pool = [(keys[(5 * i) % 12], 0) for i in range(17)]       # keys repeat
        pool[3] = (keys[0] + b"-", 0)
        pool[8] = pool[7]
        for n, launches in ((0, 0), (1, 1), (8, 1), (9, 3), (17, 5)):
            _exp, raw, delta = check_batch(d, pool[:n], path="dev")
            # every sub-batch launches once; all but the last launch again
            # for their values once the reply is known to fit
            assert delta["get_batch_launches"] == launches, (n, delta)
            assert struct.unpack_from("<I", raw, 0) == (n,)
        rc, ln, tot, out, ok = raw_call(d.p, [], 0, 4)
        assert (rc, ln, tot, out, ok) == (OK, 4, 0, b"\x00\x00\x00\x00", True)
        assert d.p.get_batch([]) == (OK, [], b"\x00\x00\x00\x00")
    finally:
        d.close()


# ---- 5. rounds and host path -------------------------------------------------
def test_rounds_and_host_path():
    ns = b"/registry/rd"
    arena = 16384
    d = bw.open_dual(KB_ARENA_BYTES=arena)
    try:
        vlens = [6000, 6000, 6000, 0, 6000, 20001, 6000, 12000, 100, 16384, 7]
        keys = [skey(ns, i, 24 + i) for i in range(len(vlens))]
        for i, (k, vl) in enumerate(zip(keys, vlens)):
            d.create(k, blob(i, vl))
        qs = [(k, 0) for k in keys[:3]] + [(keys[0] + b"-", 0)] + \
             [(k, 0) for k in keys[3:]]
        lens = vlens[:3] + [0] + vlens[3:]
        m = plan_model([ln > 0 or i == 4 for i, ln in enumerate(lens)], lens, arena)
        assert len(m["rounds"]) >= 3 and m["n_host"] == 1
        exp, raw, delta = check_batch(d, qs, path=None)
        assert [len(kv.value) if kv else 0 for _, _, kv in exp] == lens
        assert delta["get_batch_q_host"] == 1, delta
        assert delta["get_batch_q_dev"] == len(qs) - 1, delta
        # one launch per round: the first round rides on the sizing launch
        assert delta["get_batch_launches"] == len(m["rounds"]) == 6, (delta, m)
        assert delta["get_batch_bytes"] == sum(lens) - 20001, delta
        # the host-path query first: its sub-batch's launch serves no round
        qs2 = [qs[6]] + qs[:6]
        lens2 = [lens[6]] + lens[:6]
        m2 = plan_model([ln > 0 for ln in lens2], lens2, arena)
        _exp, _raw, delta = check_batch(d, qs2, path=None)
        assert delta["get_batch_q_host"] == 1, delta
        assert delta["get_batch_launches"] == len(m2["rounds"]) + 1 == 3, (delta, m2)
        # no_values needs neither rounds nor the host path
        _exp, _raw, delta = check_batch(d, qs, no_values=True, path="dev")
        assert delta["get_batch_launches"] == 1 and delta["get_batch_bytes"] == 0
    finally:
        d.close()


# ---- 6. ENOBUF ---------------------------------------------------------------
def test_enobuf(world):
    d, info = world
    qs = [(k, 0) for k in info["keys"][:60]] + [(info["keys"][0] + b"-", 0)]
    n = len(qs)
    rc, required, total, fresh, ok = raw_call(d.p, qs, 0, 1 << 20)
    assert rc == OK and ok and total > 0
    fresh = fresh[:required]
    assert required > 4 + 32 * n
    assert fresh == expected_reply([d.o.get(k, r) for k, r in qs])
    for cap in (required - 1, 4 + 32 * n - 1, 3, 0):
        before = bw.perf(d.p)
        rc, out_len, _tot, out, ok = raw_call(d.p, qs, 0, cap)
        after = bw.perf(d.p)
        assert rc == ENOBUF, (cap, rc)
        assert out_len == required, (cap, out_len, required)
        assert ok and out == b"\xc3" * cap, cap          # buffer and canary
        assert after["get_batch_bytes"] == before["get_batch_bytes"]   # no value D2H
        assert after["get_launches"] == before["get_launches"]
        rc, out_len, tot2, out, ok = raw_call(d.p, qs, 0, required)
        assert (rc, out_len, tot2, ok) == (OK, required, total, True)
        assert out == fresh


# ---- 7. flags ----------------------------------------------------------------
def test_no_values_and_bad_flags(world):
    d, info = world
    vers = info["vers"]
    qs = [(k, r) for k in info["keys"][::9]
          for r in (0, vers[k][0], vers[k][0] - 1)]      # the last: before the key
    exp, raw, _delta = check_batch(d, qs, no_values=True, path="dev")
    assert len(raw) == 4 + 32 * len(qs)
    assert sum(kv is not None for _, _, kv in exp) > 100
    assert any(kv is None for _, _, kv in exp)
    assert any(kv and kv.value for _, _, kv in exp)      # values were there to drop
    for flags in (2, 3, 4, 1 << 30, -1):
        before = bw.perf(d.p)
        rc, ln, tot, out, ok = raw_call(d.p, qs[:3], flags, 1 << 12)
        assert (rc, ln, tot, ok) == (INVALID_ARG, 0, 0, True), flags
        assert out == b"\xc3" * (1 << 12)
        after = bw.perf(d.p)
        assert after["get_batch_launches"] == before["get_batch_launches"]


# ---- 8. interleaving ---------------------------------------------------------
def test_interleaved_with_other_calls(world):
    d, info = world
    rq = info["qs"]
    cur = d.p.current_rev()
    exp = bw.expected(d, rq, cur)
    winners = sum(min(len(e), q[3]) if q[3] else len(e) for q, e in zip(rq, exp))
    gq = [(k, r) for k in info["keys"][5:400:7] for r in (0, info["hist"][0])]
    tot, _ = bw.bench_step(d.p, rq, [], 4)           # stays in flight
    check_batch(d, gq, path="dev")                   # collects it first
    assert bw.last_range(d.p, 0) == []               # the arena holds values now
    tot, _ = bw.bench_step(d.p, rq, [], 4)
    assert tot == 0                                  # nothing pending before it
    check_batch(d, gq[:9], path="dev")
    tot, _ = bw.bench_step(d.p, rq, [], 4)
    tot2, _ = bw.bench_step(d.p, rq, [], 4)          # reports the step before
    assert tot2 == winners, (tot2, winners)
    bw.sync(d.p)
    bw.check_records(rq, exp, bw.last_range(d.p, 0))
    # next to kb_list_batch, kb_get and kb_list (Dual asserts oracle parity)
    lq = rq[:12]
    rc, res1, sec1 = d.p.list_batch(lq)
    assert rc == OK
    check_batch(d, gq, path="dev")
    rc, res2, sec2 = d.p.list_batch(lq)
    assert rc == OK and sec2 == sec1
    for k, r in gq[:6]:
        d.get(k, r)
    check_batch(d, gq[:30], path="dev")
    for s, e, r, lim in lq[:4]:
        d.list(s, e, r, lim)
    assert bw.bench_range(d.p, rq, 0) == winners
    bw.check_records(rq, exp, bw.last_range(d.p, 0))
    check_batch(d, gq[:30], path="dev")
    assert bw.last_range(d.p, 0) == []


# ---- 9. seeded random --------------------------------------------------------
def test_seeded_random():
    rng = random.Random(7)
    ns = b"/registry/rnd"
    keys = [skey(ns, i, 22 + (i * 5) % 19) for i in range(150)]
    keys += [skey(ns, 900 + i, L) for i, L in enumerate((96, 97, 130, 300))]
    d = bw.open_dual()
    try:
        live, touched, revs = {}, set(), [d.p.current_rev()]
        for op in range(2000):
            k = keys[rng.randrange(len(keys))]
            v = blob(op, VLENS[rng.randrange(len(VLENS) - 8)])
            touched.add(k)
            if k not in live:
                r = d.create(k, v)
                if r.succeeded:
                    live[k] = r.header_revision
            elif rng.random() < 0.3:
                if d.delete(k, live[k]).succeeded:
                    del live[k]
            else:
                r = d.update(k, v, live[k])
                if r.succeeded:
                    live[k] = r.header_revision
            if op % 100 == 0:
                revs.append(d.p.current_rev())
        cur = d.p.current_rev()
        qs = []
        for k in sorted(touched):
            qs.append((k, 0))
            qs += [(k, rng.choice(revs + [rng.randrange(revs[0], cur + 3)]))
                   for _ in range(3)]
        rng.shuffle(qs)
        exp, _raw, _delta = check_batch(d, qs, path="dev")
        assert sum(kv is None for _, _, kv in exp) > 20
        assert sum(kv is not None for _, _, kv in exp) > 200
        d.diff_dump()
    finally:
        d.close()
