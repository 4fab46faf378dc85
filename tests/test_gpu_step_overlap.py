"""The pipelined bench step (kb_bench_step, mode bit 2) without a stream drain
(DESIGN.md §5.1f): batch i is queued before batch i-1 is collected, so the
counters of a batch live in one of two slots; gets, ranges and key tails go up
in one staged copy, delta rows in one more; the range counters are zeroed by
the bounds kernel; the event ring is pushed without waiting for the stream;
value bytes are appended to one heap only. Every result is compared with the
CPU oracle."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import benchwire as bw
import parity
from kbclient import OK

pytestmark = pytest.mark.gpu

parity.small_env()

NS = [b"/registry/pods/ns-%02d" % i for i in range(4)]
PER_NS = 120
VLENS = [0, 1, 15, 16, 17, 100, 512, 1025]
# a key longer than the 96-byte key column (its tail lives in the spill heap)
LONGK = NS[1] + b"/long-" + b"y" * 120


def val(tag, n):
    return bytes((tag * 11 + j * 7 + (j >> 8)) % 200 + 0x30 for j in range(n))


def key(ns, i):
    return ns + b"/obj-%04d" % i


def build(d):
    """480 keys + one long key, a second version of every fifth, every
    eleventh deleted (tombstones). Deterministic: every store built here
    holds the same rows at the same revisions."""
    keys = [key(ns, i) for ns in NS for i in range(PER_NS)] + [LONGK]
    rev = {}

    def txn(ops):
        for c0 in range(0, len(ops), 200):
            chunk = ops[c0:c0 + 200]
            out = bw.dual_txn(d, chunk)
            assert all(out)
            for (k, _p, _v), r in zip(chunk, out):
                rev[k] = r

    txn([(k, 0, val(i, VLENS[i % 8])) for i, k in enumerate(keys)])
    txn([(k, rev[k], val(i + 3, VLENS[(i + 1) % 8]))
         for i, k in enumerate(keys) if i % 5 == 2])
    dead = [k for i, k in enumerate(keys[:-1]) if i % 11 == 7]
    tomb = {}
    for (k, r) in zip(dead, bw.dual_del(d, [(k, 0) for k in dead])):
        assert r
        tomb[k] = r
    d.count(NS[0] + b"/", NS[0] + b"0")   # device state current
    deadset = set(dead)
    return {"keys": keys, "rev": rev, "dead": dead, "tomb": tomb,
            "live": [k for k in keys[:-1] if k not in deadset]}


def drain(d, idx):
    """Poll a watcher pair until it is empty -> all events, in order."""
    evs = []
    for _ in range(16):
        got = d.poll(idx)
        if not got:
            break
        evs += got
    return evs


def winners_of(qs, exp):
    return sum(min(len(e), q[3]) if q[3] else len(e) for q, e in zip(qs, exp))


def apply_oracle(d, ops, out, rev):
    """The step's txns through the oracle's serial Update; same revisions."""
    for (k, prev, v), nr in zip(ops, out):
        ro = d.o.update(k, v, prev)
        assert (ro.header_revision if ro.succeeded else 0) == nr, (k, prev, ro, nr)
        if nr:
            rev[k] = nr


def step(d, info, qs, ops, mode):
    """One kb_bench_step + the oracle replay -> (total, revisions, expected
    records of qs at the pre-step snapshot)."""
    exp = bw.expected(d, qs, d.p.current_rev())
    tot, out = bw.bench_step(d.p, qs, ops, mode)
    apply_oracle(d, ops, out, info["rev"])
    return tot, out, exp


def pool_queries(ns_keys):
    """Queries whose first covers every txn key of a step (all in NS[0])."""
    qs = [(NS[0] + b"/", NS[0] + b"0", 0, 0),
          (NS[1] + b"/", NS[1] + b"0", 0, 7),
          (LONGK, LONGK + b"0", 0, 0)]
    qs += [(k, k + b"0", 0, 0) for k in ns_keys[:20]]
    qs += [(NS[2] + b"/", NS[2] + b"0", 0, 0), (NS[3] + b"/", NS[3] + b"0", 0, 1)]
    qs += [(k + b"-", k + b"-z", 0, 0) for k in ns_keys[20:35]]   # empty ranges
    assert len(qs) == 40
    return qs


# ---- 1. slot rotation --------------------------------------------------------
NQS = [1, 3, 40, 2, 0, 1]
NTX = [8, 1, 0, 8, 1, 8]


def run_sequence(mode):
    d = bw.open_dual()
    try:
        info = build(d)
        live0 = [k for k in info["live"] if k.startswith(NS[0] + b"/")]
        pool = pool_queries(live0)
        used = 0
        totals, winners, revs, batches = [], [], [], []
        for nq, ntx in zip(NQS, NTX):
            ups = live0[used:used + ntx]
            used += ntx
            ops = [(k, info["rev"][k], val(used + i, VLENS[(used + i) % 8]))
                   for i, k in enumerate(ups)]
            qs = pool[:nq]
            tot, out, exp = step(d, info, qs, ops, mode)
            assert all(out), (mode, nq, out)
            totals.append(tot)
            winners.append(winners_of(qs, exp))
            revs.append(out)
            batches.append((qs, exp))
            if mode == 0 and nq:
                bw.check_records(qs, exp, bw.last_range(d.p, 0))
        if mode == 4:
            # step k reports the winners of step k-1
            assert totals == [0] + winners[:-1], (totals, winners)
            bw.sync(d.p)
            qs, exp = batches[-1]
            bw.check_records(qs, exp, bw.last_range(d.p, 0))
            # ... and that snapshot predates the step's own txns
            assert bw.expected(d, qs, d.p.current_rev()) != exp
            # an empty batch leaves the last non-empty one in place
            tot, _out, _exp = step(d, info, [], [], 4)
            assert tot == 0
            bw.sync(d.p)
            bw.check_records(qs, exp, bw.last_range(d.p, 0))
        else:
            assert totals == winners
        assert winners[2] > winners[0] > 0 and winners[4] == 0
        d.list(NS[0] + b"/", NS[0] + b"0", 0, 0)
        d.diff_dump()
        return winners, revs
    finally:
        d.close()


def test_slot_rotation():
    w4, r4 = run_sequence(4)
    w0, r0 = run_sequence(0)
    assert w4 == w0 and r4 == r0


# ---- 2. foreign reads between pipelined steps --------------------------------
def test_foreign_reads_between_steps():
    d = bw.open_dual()
    try:
        info = build(d)
        live = info["live"]
        widx = d.watch(NS[0] + b"/", 0)
        lq = [(NS[1] + b"/", NS[1] + b"0", 0, 0), (NS[0] + b"/", NS[0] + b"0", 0, 5),
              (LONGK, LONGK + b"0", 0, 0)]
        gq = [(live[3], 0), (info["dead"][0], 0), (LONGK, 0), (b"/registry/pods/none", 0)]

        def f_list():
            d.list(NS[0] + b"/", NS[0] + b"0", 0, 0)
            d.list(NS[2] + b"/", NS[2] + b"0", 0, 3)

        def f_list_batch():
            rc, res, _raw = d.p.list_batch(lq)
            assert rc == OK
            for q, (st, rp) in zip(lq, res):
                lo = d.o.list(*q)
                assert (st, rp.header_revision, rp.more, rp.kvs) == \
                       (lo.status, lo.header_revision, lo.more, lo.kvs), q

        def f_get_batch():
            rc, res, _raw = d.p.get_batch(gq)
            assert rc == OK
            assert res == [d.o.get(k, r) for k, r in gq]

        def f_watch_poll():
            assert len(d.poll(widx)) > 0

        def f_compact():
            d.compact(d.p.current_rev() - 5)

        used = 0
        for foreign in (f_list, f_list_batch, f_get_batch, f_watch_poll, f_compact):
            ups = [k for k in live[used:used + 6]]
            used += 6
            qs = [(k, k + b"0", 0, 0) for k in ups[:3]] + \
                [(NS[0] + b"/", NS[0] + b"0", 0, 0), (NS[1] + b"/", NS[1] + b"0", 0, 7)]
            ops = [(k, info["rev"][k], val(used + i, VLENS[(used + i) % 8]))
                   for i, k in enumerate(ups)]
            tot, out, _exp = step(d, info, qs, ops, 4)
            assert tot == 0 and all(out), foreign.__name__
            foreign()          # collects the batch in flight before it runs
            qs2 = qs[1:] + [(NS[3] + b"/", NS[3] + b"0", 0, 0)]
            tot, out, exp2 = step(d, info, qs2, [], 4)
            assert tot == 0, (foreign.__name__, tot)   # nothing left to collect
            bw.sync(d.p)
            bw.check_records(qs2, exp2, bw.last_range(d.p, 0))
        d.poll(widx)
        d.list(NS[0] + b"/", NS[0] + b"0", 0, 0)
        d.diff_dump()
    finally:
        d.close()


# ---- 3. upload layout --------------------------------------------------------
@pytest.mark.parametrize("validate", [0, 1])
@pytest.mark.parametrize("regime", ["small", "big"])
def test_upload_layout(regime, validate):
    d = bw.open_dual(KB_VALIDATE_DN=validate, KB_FLUSH_ROWS=1 << 16)
    try:
        info = build(d)
        if regime == "small":
            bw.flush(d.p)      # delta empty: delta + new rows <= 2048
        else:
            extra = [b"/registry/pods/pre/obj-%05d" % i for i in range(700)]
            for c0 in range(0, len(extra), 350):
                assert all(bw.dual_txn(d, [(k, 0, val(i, 32)) for i, k in
                                           enumerate(extra[c0:c0 + 350])]))
            d.count(NS[0] + b"/", NS[0] + b"0")
            assert bw.perf(d.p)["delta_rows"] > 2048
        rev, live, dead = info["rev"], info["live"], info["dead"]
        newk = b"/registry/pods/ns-02/new-" + b"n" * 100      # create, > 96 B
        batches = [
            [(LONGK, rev[LONGK], val(1, 100))],                 # 1 op, long key
            [(live[0], rev[live[0]], val(2, 512)),
             (live[1], rev[live[1]] - 1, val(3, 17)),           # stale prev -> 0
             (dead[0], rev[dead[0]], val(4, 16))],              # on a tombstone
            [(newk, 0, val(5, 1025))],                          # create
            [(dead[1], 0, val(6, 15)),                          # create over tomb
             (live[2], rev[live[2]], b""),
             (LONGK, 1, val(7, 1))],                            # stale, long key
        ]
        before = bw.perf(d.p)
        outs = []
        for ops in batches:
            qs = [(k, k + b"0", 0, 0) for k, _p, _v in ops]
            tot, out, _exp = step(d, info, qs, ops, 4)
            outs.append(out)
            assert len(out) in (1, 3)
        assert outs[0][0] and outs[2][0]
        assert outs[1][0] and not outs[1][1] and not outs[1][2]
        assert outs[3][0] and outs[3][1] and not outs[3][2]
        # the staged rows of the last step merge with the next step's upload
        qs = [(NS[0] + b"/", NS[0] + b"0", 0, 0), (newk, newk + b"0", 0, 0),
              (LONGK, LONGK + b"0", 0, 0)]
        _tot, _out, exp = step(d, info, qs, [], 4)
        bw.sync(d.p)
        bw.check_records(qs, exp, bw.last_range(d.p, 0))
        after = bw.perf(d.p)
        merged = after["merges"] - before["merges"]
        assert merged == 4, (before, after)
        if regime == "small":
            assert after["merge_small"] - before["merge_small"] == 4, after
        else:
            assert after["merge_small"] == before["merge_small"], after
            assert after["merge_insert"] - before["merge_insert"] == 4, after
        if not validate:
            assert after["merges_async"] - before["merges_async"] == 4, after
        d.get(LONGK)
        d.get(newk)
        d.list(NS[0] + b"/", NS[0] + b"0", 0, 0)
        d.diff_dump()
    finally:
        d.close()


# ---- 4. counter zeroing ------------------------------------------------------
def test_counters_zeroed_per_batch():
    d = bw.open_dual()
    try:
        build(d)
        qs = [(NS[0] + b"/", NS[0] + b"0", 0, 0), (NS[1] + b"/", NS[1] + b"0", 0, 7),
              (LONGK, LONGK + b"0", 0, 0)]
        deltas = []
        for mode in (0, 0, 4, 4):
            p0 = bw.perf(d.p)
            bw.bench_step(d.p, qs, [], mode)
            bw.sync(d.p)        # a pipelined batch is counted when collected
            p1 = bw.perf(d.p)
            deltas.append((p1["rows_scanned"] - p0["rows_scanned"],
                           p1["bytes_gathered"] - p0["bytes_gathered"],
                           p1["winners"] - p0["winners"]))
        # the same batch, the same counts: a counter that is not reset would
        # double from run to run
        assert len(set(deltas)) == 1, deltas
        assert all(x > 0 for x in deltas[0]), deltas
    finally:
        d.close()


# ---- 5. event ring without a drain ------------------------------------------
def test_event_ring_push_in_flight():
    d = bw.open_dual()
    try:
        info = build(d)
        rev0 = d.p.current_rev()
        w_ns = d.watch(NS[0] + b"/", 0)
        w_all = d.watch(b"/registry/pods/", 0)
        live = info["live"]
        assert len(live) >= 400
        qs = [(ns + b"/", ns + b"0", 0, 0) for ns in NS] * 4
        prev = 0
        for s in range(4):      # the 300-event pump falls inside the third step
            ups = live[s * 100:(s + 1) * 100]
            ops = [(k, info["rev"][k], val(s * 100 + i, VLENS[i % 8]))
                   for i, k in enumerate(ups)]
            tot, out, exp = step(d, info, qs, ops, 4)
            assert all(out) and tot == prev
            prev = winners_of(qs, exp)
        ev_ns = drain(d, w_ns)
        ev_all = drain(d, w_all)
        assert len(ev_all) == 400 and 0 < len(ev_ns) < 400
        assert [e.revision for e in ev_all] == sorted(e.revision for e in ev_all)
        # a watcher opened now at an old revision catches up from the device ring
        late = d.watch(NS[1] + b"/", rev0 + 150)
        assert late is not None
        ev_late = drain(d, late)
        assert 0 < len(ev_late) < 400
        bw.sync(d.p)
        d.list(NS[0] + b"/", NS[0] + b"0", 0, 0)
        d.diff_dump()
    finally:
        d.close()


# ---- 6. heap after compaction ------------------------------------------------
def test_heap_after_two_compactions():
    d = bw.open_dual()
    try:
        info = build(d)            # writes, a key > 96 B, tombstones
        rev, live = info["rev"], info["live"]

        def writes(tag, ks):
            ops = [(k, rev[k], val(tag + i, VLENS[(tag + i) % 8]))
                   for i, k in enumerate(ks)]
            out = bw.dual_txn(d, ops)
            assert all(out)
            for (k, _p, _v), r in zip(ops, out):
                rev[k] = r

        p0 = bw.perf(d.p)
        d.compact(d.p.current_rev() - 1)
        writes(100, live[:50] + [LONGK])
        assert all(bw.dual_del(d, [(k, 0) for k in live[50:55]]))
        d.compact(d.p.current_rev() - 1)
        writes(200, live[10:40] + [LONGK])
        assert bw.perf(d.p)["compacts"] - p0["compacts"] >= 2
        for k in info["keys"]:
            d.get(k)               # value bytes equal the oracle's
        for ns in NS:
            d.list(ns + b"/", ns + b"0", 0, 0)
        d.get(LONGK, rev[LONGK])
        d.diff_dump()
    finally:
        d.close()
