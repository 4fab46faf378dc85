"""Byte-check of the batched Range hot path (kb_bench_range / kb_bench_step):
every record each query produced, read back through kb_test_last_range from
the device arena (src 0) and from the pinned buffers of the pipelined D2H
(src 1), against the CPU oracle's List of the same range and revision."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import benchwire as bw
import parity

pytestmark = pytest.mark.gpu

parity.small_env()

NS = [b"/registry/pods/ns-%02d" % i for i in range(6)]
PER_NS = 200
VLENS = [0, 1, 15, 16, 17, 100, 512, 4097]
# 96-byte prefix shared by keys of 96, 97 and 300 bytes (tails live in the
# key-spill heap; every compare of these keys reaches the tail)
P96 = NS[3] + b"/long-" + b"x" * (96 - len(NS[3]) - 6)
LONG = [P96, P96 + b"a", P96 + b"a" * 204, P96 + b"b", P96 + b"b" * 204]
# one namespace of equal 512-byte values: three ranges over it overflow a
# 16 KiB per-query arena (test_batch_arena_overflow)
FAT = b"/registry/pods/ns-fat"
FAT_N = 120

_BLOB = np.random.default_rng(0xB1B).integers(
    0x30, 0x7b, size=1 << 16, dtype=np.uint8).tobytes()


def val(tag: int, n: int) -> bytes:
    o = (tag * 131) % (len(_BLOB) - 4200)
    return _BLOB[o:o + n]


def key(ns, i):
    return ns + b"/obj-%04d" % i


def build(d):
    """~3000 rows through kb_bench_txn / kb_bench_del batches on the product
    and the serial protocol on the oracle. Deterministic: every store built
    here holds the same rows at the same revisions."""
    assert len(P96) == 96 and [len(k) for k in LONG] == [96, 97, 300, 97, 300]
    keys = [key(ns, i) for ns in NS for i in range(PER_NS)] + LONG
    fat = [FAT + b"/obj-%04d" % i for i in range(FAT_N)]
    rev = {}

    def txn(ops):
        for c0 in range(0, len(ops), 400):
            chunk = ops[c0:c0 + 400]
            out = bw.dual_txn(d, chunk)
            assert all(out), "every fixture op must succeed"
            for (k, _p, _v), r in zip(chunk, out):
                rev[k] = r

    txn([(k, 0, val(i, VLENS[i % 8])) for i, k in enumerate(keys)])
    txn([(k, 0, val(i, 512)) for i, k in enumerate(fat)])
    r1 = d.p.current_rev()
    for gen, step in enumerate((4, 8, 16, 32)):   # keys with 2..5 versions
        txn([(k, rev[k], val(i + 7 * gen + 1, VLENS[(i + gen + 1) % 8]))
             for i, k in enumerate(keys) if i % step == 1])
        if step == 8:
            r2 = d.p.current_rev()
    dead = [k for i, k in enumerate(keys) if i % 7 == 3]
    for c0 in range(0, len(dead), 100):
        assert all(bw.dual_del(d, [(k, 0) for k in dead[c0:c0 + 100]]))
    r3 = d.p.current_rev()
    txn([(k, 0, val(i + 99, VLENS[(i + 3) % 8]))      # recreate over tombstones
         for i, k in enumerate(dead) if i % 3 == 0])
    # a last small batch stays in the delta run (KB_FLUSH_ROWS=512)
    deadset = set(dead)
    live = [k for k in keys[PER_NS:2 * PER_NS] if k not in deadset][:60]
    txn([(k, rev[k], val(i + 555, VLENS[(i + 5) % 8])) for i, k in enumerate(live)])
    d.count(NS[0] + b"/", NS[0] + b"0")   # device state current
    p = bw.perf(d.p)
    assert p["base_rows"] > 0 and p["delta_rows"] > 0, p
    assert 2500 <= p["base_rows"] + p["delta_rows"] <= 4000, p
    return {"keys": keys, "fat": fat, "rev": rev, "dead": dead,
            "hist": [r1, r2, r3], "cur": d.p.current_rev()}


def make_queries(info, n=150, seed=5):
    """n queries of the shapes the bench path has to get right."""
    rng = np.random.default_rng(seed)
    keys, cur = info["keys"], info["cur"]
    revs = [0, cur - 1] + info["hist"]
    limits = [0, 1, 7, 500]
    qs = []

    def add(s, e):
        i = len(qs)
        qs.append((s, e, revs[i % 5], limits[(i // 5 + i) % 4]))

    for ns in NS:                                   # whole namespaces
        add(ns + b"/", ns + b"0")
        add(ns + b"/", ns + b"0")
    add(FAT + b"/", FAT + b"0")
    add(P96, P96 + b"c")                            # the five long keys
    add(LONG[1], LONG[4])                           # 97-byte start, 300-byte end
    add(LONG[2], LONG[2] + b"0")                    # one 300-byte key
    add(NS[3] + b"/long-", LONG[0] + b"0")          # ends between 96 and 97
    while len(qs) < n - 10:
        kind = len(qs) % 5
        ns = NS[int(rng.integers(len(NS)))]
        a = int(rng.integers(PER_NS - 1))
        b = int(rng.integers(a + 1, min(PER_NS, a + 60) + 1))
        if kind == 0:                               # on keys
            add(key(ns, a), key(ns, b))
        elif kind == 1:                             # between keys
            add(key(ns, a) + b"-", key(ns, b) + b"-")
        elif kind == 2:                             # single key
            add(key(ns, a), key(ns, a) + b"0")
        elif kind == 3:                             # empty: between two keys
            add(key(ns, a) + b"-", key(ns, a) + b"-z")
        else:                                       # on a key, ends between
            add(key(ns, a), key(ns, b - 1) + b"-")
    for i in range(n - len(qs)):                    # repeats
        qs.append(qs[i * 3 + 1])
    assert len(qs) == n
    return qs


@pytest.fixture(scope="module")
def world():
    d = bw.open_dual()
    try:
        info = build(d)
        info["qs"] = make_queries(info)
        info["cache"] = {}
        info["exp"] = bw.expected(d, info["qs"], info["cur"], info["cache"])
        yield d, info
    finally:
        d.close()


def hook_rc(store, src):
    out_len = C.c_size_t()
    buf = C.create_string_buffer(16)
    return store._f("test_last_range")(C.c_void_p(store.h), C.c_int(src), buf,
                                       C.c_size_t(16), C.byref(out_len))


def run_and_check(d, qs, exp, mode, allow_overflow=()):
    tot = bw.bench_range(d.p, qs, mode)
    got0 = bw.last_range(d.p, 0)
    bw.check_records(qs, exp, got0, keys_only=bool(mode & 2),
                     allow_overflow=allow_overflow)
    assert tot == sum(min(w, q[3]) if q[3] else w
                      for q, (w, _t, _b, _o, _r) in zip(qs, got0))
    if mode & 1:
        got1 = bw.last_range(d.p, 1)
        bw.check_records(qs, exp, got1, keys_only=bool(mode & 2),
                         allow_overflow=allow_overflow)
        assert got1 == got0
    else:
        assert hook_rc(d.p, 1) == 13  # KB_EINTERNAL: batch ran without d2h
    return got0


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_batch_records_match_oracle(world, mode):
    d, info = world
    qs, exp = info["qs"], info["exp"]
    assert len(qs) == 150
    # the query set really has every shape it claims
    assert {q[3] for q in qs} == {0, 1, 7, 500}
    assert len({q[2] for q in qs}) == 5
    assert sum(1 for e in exp if not e) >= 10
    assert sum(1 for q, e in zip(qs, exp) if q[3] and len(e) > q[3]) >= 10
    assert len(set(qs)) < len(qs)
    got = run_and_check(d, qs, exp, mode)
    if mode & 2:
        assert all(v == b"" for g in got for _r, _k, v in g[4])
        # keys-only records carry no value bytes at all
        assert all(g[2] == sum(16 + bw.pad16(len(k)) for _r, k, _v in g[4])
                   for g in got)
    else:
        vl = {len(v) for g in got for _r, _k, v in g[4]}
        assert set(VLENS) <= vl, vl
    assert {len(k) for g in got for _r, k, _v in g[4]} >= {96, 97, 300}


KNOBS = {"gather_mode2": {"KB_GATHER_MODE": 2}, "gw1": {"KB_GATHER_GW": 1},
         "gw64": {"KB_GATHER_GW": 64}, "scan_t256": {"KB_SCAN_T": 256},
         "gather_t64": {"KB_GATHER_T": 64}}


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_batch_records_knobs(world, knob):
    _d, info = world
    d = bw.open_dual(**KNOBS[knob])
    try:
        mine = build(d)
        assert mine["cur"] == info["cur"] and mine["hist"] == info["hist"]
        run_and_check(d, info["qs"], info["exp"], 1)
    finally:
        d.close()


def test_step_modes(world):
    _d, info = world
    d = bw.open_dual()
    try:
        mine = build(d)
        rev, dead = mine["rev"], set(mine["dead"])
        live = [k for k in mine["keys"] if k not in dead]
        base_qs = [q for q in info["qs"] if q[3] != 1][:40]
        used = 0
        for mode in (0, 1, 4):
            last = None
            prev_winners = 0
            for step in range(3):
                ups = live[used:used + 8]
                used += 8
                # every updated key sits inside a current-revision query
                qs = base_qs + [(k, k + b"0", 0, 0) for k in ups[:4]] + \
                    [(ups[4], ups[7] + b"0", 0, 7)]
                cur = d.p.current_rev()
                exp = bw.expected(d, qs, cur)
                ops = [(k, rev[k], val(used + i, VLENS[(used + i) % 8]))
                       for i, k in enumerate(ups)]
                tot, out = bw.bench_step(d.p, qs, ops, mode)
                assert all(out), (mode, step, out)
                for (k, prev, v), nr in zip(ops, out):
                    ro = d.o.update(k, v, prev)
                    assert ro.succeeded and ro.header_revision == nr
                    rev[k] = nr
                winners = sum(min(len(e), q[3]) if q[3] else len(e)
                              for q, e in zip(qs, exp))
                if mode == 4:
                    # a pipelined step reports the previous step's winners
                    assert tot == prev_winners, (step, tot, prev_winners)
                    prev_winners = winners
                    last = (qs, exp)
                    continue
                assert tot == winners
                bw.check_records(qs, exp, bw.last_range(d.p, 0))
                if mode == 1:
                    bw.check_records(qs, exp, bw.last_range(d.p, 1))
            if mode == 4:
                bw.sync(d.p)
                qs, exp = last
                bw.check_records(qs, exp, bw.last_range(d.p, 0))
                # ... and that snapshot predates the step's own txns
                after = bw.expected(d, qs, d.p.current_rev())
                assert after != exp
        d.list(NS[0] + b"/", NS[0] + b"0", 0, 0)
        d.diff_dump()
    finally:
        d.close()


def test_pipelined_slots_not_stale(world):
    d, info = world
    keys, cur = info["keys"], info["cur"]
    single = [(k, k + b"0", 0, 0) for k in keys]
    spaces = [(ns + b"/", ns + b"0", 0, 0) for ns in NS]
    batches = [
        single[3:13],                                   # small   -> one slot
        single[200:290] + spaces[:1],                   # large   -> the other
        single[400:405],                                # small   -> first again
        spaces + [(ns + b"/", ns + b"0", cur - 1, 0) for ns in NS]
        + single[600:700],                              # larger  -> regrows it
        single[1001:1002],                              # tiny
    ]
    sizes = []
    for qs in batches:
        exp = bw.expected(d, qs, cur, info["cache"])
        bw.bench_range(d.p, qs, 1)
        got = bw.last_range(d.p, 1)
        bw.check_records(qs, exp, got)
        sizes.append(sum(g[2] for g in got))
    # the fourth batch outgrows what the second left allocated for its slot
    # (buffers grow to 1.5x the need), so that slot is freed and regrown
    assert sizes[3] > 1.5 * sizes[1] > 1.5 * sizes[0] > 0, sizes
    assert 0 < sizes[4] < sizes[2] < sizes[1], sizes
    bw.sync(d.p)


def test_batch_arena_overflow(world):
    _d, info = world
    d = bw.open_dual(KB_ARENA_BYTES=1 << 20)
    try:
        mine = build(d)
        cur, fat = mine["cur"], mine["fat"]
        assert cur == info["cur"]
        qcap = (1 << 20) // 64

        def need(e, limit):
            return sum(16 + bw.pad16(len(k)) + bw.pad16(len(v))
                       for _r, k, v in (e[:limit + 1] if limit else e))

        # the other 61: queries whose oracle records fit a 16 KiB region
        small = [q for q, e in zip(info["qs"], info["exp"])
                 if need(e, q[3]) <= qcap][:61]
        assert len(small) == 61 and sum(1 for q in small if q[3] == 0) >= 10
        over = {5: (FAT + b"/", FAT + b"0", 0, 0),
                31: (FAT + b"/", FAT + b"0", cur - 1, 0),
                63: (fat[10], fat[110], 0, 500)}
        qs = list(small)
        for pos in sorted(over):
            qs.insert(pos, over[pos])
        assert len(qs) == 64
        exp = bw.expected(d, qs, cur, info["cache"])
        assert [len(exp[i]) for i in sorted(over)] == [120, 120, 100]
        assert all(need(exp[i], qs[i][3]) > 3 * qcap for i in over)
        got = run_and_check(d, qs, exp, 1, allow_overflow=set(over))
        for i in over:
            w, _t, nbytes, ovf, recs = got[i]
            assert ovf and not recs
            assert nbytes == need(exp[i], qs[i][3]) > qcap  # why it overflowed
    finally:
        d.close()
