"""The engine regimes the benchmark runs in but the parity suite never
selected: the async (unvalidated) delta merge, the big inverted merge and the
inverted insert on a large delta run, capacity folds, an all-delta store, the
tile loop of the winner scan over sparse winners, and the 64-ary search at
the run sizes where its rounds change. Every case proves from the
kb_perf_json counters that it reached the path it names; results are compared
with the CPU oracle byte for byte (parity.Dual)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import benchwire as bw
import parity

pytestmark = pytest.mark.gpu

parity.small_env()

NS = [b"/registry/pods/ns-%02d" % i for i in range(8)]
BRANCHES = ("merge_small", "merge_insert", "merge_big", "merge_empty", "folds")


def v(tag, n=40):
    return ((b"%08d-" % tag) * (n // 9 + 1))[:n]


# ---- the shared deterministic workload ------------------------------------
def run_workload(d, mid_compact=True, after_bulk=None, each_round=None):
    """Bulk load + 6 rounds of mixed batches and reads; returns the perf
    snapshots taken after every batch and read block."""
    rng = np.random.default_rng(0xE61)
    trace = [bw.perf(d.p)]
    snap = lambda: trace.append(bw.perf(d.p))  # noqa: E731
    rev, tomb, marks = {}, [], []
    nfresh = 0
    for b in range(4):                     # bulk: 4 x 1000 creates, >= 8000 rows
        ops = [(NS[i % 8] + b"/obj-%05d" % i, 0, v(i))
               for i in range(b * 1000, (b + 1) * 1000)]
        for (k, _p, _v), r in zip(ops, bw.dual_txn(d, ops)):
            assert r
            rev[k] = r
        snap()
    d.count(NS[0] + b"/", NS[0] + b"0")
    snap()
    if after_bulk:
        after_bulk(trace)
    marks.append(d.p.current_rev())
    compacted = 0
    for rnd in range(6):
        live = sorted(rev)
        pick = [live[int(i)] for i in rng.permutation(len(live))[:660]]
        # 700 unique ops: 490 CAS with the tracked revision, 70 with a stale
        # one, 70 fresh keys, up to 70 recreates over tombstones (topped up
        # with CAS while there are fewer tombstones)
        nre = min(70, len(tomb))
        ops = [(k, rev[k], v(rnd * 7919 + i, 24 + i % 90))
               for i, k in enumerate(pick[:490])]
        ops += [(k, rev[k] - 1, b"stale") for k in pick[490:560]]
        ops += [(NS[(nfresh + i) % 8] + b"/new-%05d" % (nfresh + i), 0, v(i, 64))
                for i in range(70)]
        nfresh += 70
        ops += [(k, 0, v(rnd + i, 33)) for i, k in enumerate(tomb[:nre])]
        tomb = tomb[nre:]
        ops += [(k, rev[k], v(i, 12)) for i, k in enumerate(pick[560:630 - nre])]
        assert len(ops) == 700 and len({o[0] for o in ops}) == 700
        out = bw.dual_txn(d, ops)
        assert [i for i, r in enumerate(out) if not r] == list(range(490, 560)), \
            "exactly the stale ops fail"
        for (k, _prev, _v), r in zip(ops, out):
            if r:
                rev[k] = r
        snap()
        live = sorted(rev)
        victims = [live[int(i)] for i in rng.permutation(len(live))[:100]]
        dels = [(k, 0) for k in victims[:80]] + \
               [(k, rev[k]) for k in victims[80:90]] + \
               [(k, rev[k] - 1) for k in victims[90:]]
        outd = bw.dual_del(d, dels)
        assert all(outd[:90]) and not any(outd[90:])
        for k in victims[:90]:
            del rev[k]
            tomb.append(k)
        snap()
        cur = d.p.current_rev()
        marks.append(cur)
        old = [m for m in marks if m >= compacted]
        for i in range(12):
            ns = NS[(rnd + i) % 8]
            r = 0 if i % 2 == 0 else old[(rnd * 5 + i) % len(old)]
            d.list(ns + b"/", ns + b"0", r, (0, 1, 17, 500)[(i // 2 + i) % 4])
        snap()
        allk = sorted(rev) + tomb
        for i in range(40):
            k = allk[int(rng.integers(len(allk)))] if i % 8 else NS[i % 8] + b"/none"
            d.get(k, 0 if i % 3 else old[i % len(old)])
        d.count(NS[rnd % 8] + b"/", NS[rnd % 8] + b"0")
        d.count(b"/registry/pods/", b"/registry/pods0")
        snap()
        if each_round:
            each_round(trace)
        if rnd == 2 and mid_compact:
            compacted = marks[2]
            d.compact(compacted)
            d.diff_dump()
            snap()
    final = bw.perf(d.p)
    d.diff_dump()
    d.diff_event_log()
    return trace, final


def insert_on_big_delta(trace):
    """A delta append through k_merge_insert_inv onto a delta run of more
    than 2048 rows: between two snapshots with no fold, every merge is a
    delta append onto at least the first snapshot's delta_rows."""
    return any(a["delta_rows"] > 2048 and b["folds"] == a["folds"] and
               b["merge_insert"] > a["merge_insert"]
               for a, b in zip(trace, trace[1:]))


def big_fold_onto_base(trace):
    """A fold of a non-empty base (k_merge_rank_inv_big): more than 1024
    delta rows folded into base rows that were already there."""
    return any(a["base_rows"] > 0 and a["delta_rows"] > 1024 and
               b["folds"] > a["folds"] and b["merge_big"] > a["merge_big"]
               for a, b in zip(trace, trace[1:]))


_async_branches = {}


@pytest.mark.parametrize("validate", [0, 1], ids=["async", "validated"])
def test_bench_like_merges(validate):
    d = bw.open_dual(KB_VALIDATE_DN=validate, KB_FLUSH_ROWS=6000)
    try:
        trace, p = run_workload(d)
        if validate:
            assert p["merges_async"] == 0, p
        else:
            assert p["merges_async"] > 0, p
        assert p["merge_insert"] > 0 and insert_on_big_delta(trace), p
        assert p["merge_big"] >= p["folds"] > 0, p
        assert big_fold_onto_base(trace), p
        # a wrong row-count prediction would shift the branches the later
        # merges take; both regimes must take the same ones
        mine = tuple(p[k] for k in BRANCHES)
        other = _async_branches.setdefault("seen", mine)
        assert mine == other, (mine, other)
    finally:
        d.close()


def test_capacity_fold():
    d = bw.open_dual(KB_VALIDATE_DN=0, KB_DELTA_CAP=3000, KB_FLUSH_ROWS=100000)
    try:
        def after_bulk(trace):
            # nothing but the dn + m > delta_cap branch can have folded here:
            # no compact, no dump, and the flush threshold is out of reach
            p = trace[-1]
            assert p["folds"] > 0 and p["compacts"] == 0, p
            assert all(t["delta_rows"] <= 3000 for t in trace), trace
        trace, p = run_workload(d, after_bulk=after_bulk)
        assert p["merges_async"] > 0, p
        assert max(t["delta_rows"] for t in trace) <= 3000
    finally:
        d.close()


def test_all_delta():
    d = bw.open_dual(KB_VALIDATE_DN=0, KB_FLUSH_ROWS=1000000)
    try:
        def each_round(trace):
            p = trace[-1]
            assert p["base_rows"] == 0 and p["folds"] == 0, p
            assert p["delta_rows"] > 4096, p
        trace, p = run_workload(d, mid_compact=False, each_round=each_round)
        assert p["base_rows"] == 0 and p["delta_rows"] > 4096, p
        assert p["merges_async"] > 0 and insert_on_big_delta(trace), p
    finally:
        d.close()


# ---- sparse winners: the tile loop of scan_run_winners --------------------
TNS = b"/registry/pods/sparse"


def build_versions(d, nkeys, flush_after=False):
    """nkeys x (create + 6 updates) in one namespace, by batches."""
    keys = [TNS + b"/obj-%05d" % i for i in range(nkeys)]
    rev = {}
    for gen in range(7):
        for c0 in range(0, nkeys, 800):
            ops = [(k, rev.get(k, 0), v(gen * 100000 + c0 + i, 20 + (i + gen) % 50))
                   for i, k in enumerate(keys[c0:c0 + 800])]
            for (k, _p, _v), r in zip(ops, bw.dual_txn(d, ops)):
                assert r
                rev[k] = r
    if flush_after:
        bw.flush(d.p)
    return keys, rev


@pytest.mark.parametrize("residency", ["base", "delta", "base+delta-tombstones"])
@pytest.mark.parametrize("scan_t", [256, 1024])
def test_sparse_winner_tiles(scan_t, residency):
    flush_rows = 512 if residency == "base" else 1000000
    d = bw.open_dual(KB_SCAN_T=scan_t, KB_FLUSH_ROWS=flush_rows)
    try:
        keys, rev = build_versions(d, 600, flush_after=residency != "delta")
        before = d.p.current_rev()
        dead = [k for i, k in enumerate(keys) if i % 37]
        mid = None
        for c0 in range(0, len(dead), 300):
            assert all(bw.dual_del(d, [(k, 0) for k in dead[c0:c0 + 300]]))
            mid = mid or d.p.current_rev()
        if residency == "base":
            bw.flush(d.p)
        s, e = TNS + b"/", TNS + b"0"
        d.count(s, e)
        p = bw.perf(d.p)
        rows = 600 * 8 + len(dead)
        if residency == "base":
            assert (p["base_rows"], p["delta_rows"]) == (rows, 0), p
        elif residency == "delta":
            assert (p["base_rows"], p["delta_rows"]) == (0, rows), p
        else:  # tombstones and their revision rows sit in the delta run
            assert (p["base_rows"], p["delta_rows"]) == (4800, 2 * len(dead)), p
        span = p["base_rows"] + p["delta_rows"]
        for r in (0, before, mid):
            for limit in (1, 2, 3, 15, 16, 17, 0):
                d.list(s, e, r, limit)
        assert d.count(s, e)[2] == 600 - len(dead) == 17
        # batched read, limit 1, through the hook
        qs = [(s, e, 0, 1), (s, e, mid, 1), (keys[40], e, 0, 1)]
        exp = bw.expected(d, qs, d.p.current_rev())
        bw.bench_range(d.p, qs, 1)
        bw.check_records(qs, exp, bw.last_range(d.p, 0))
        bw.check_records(qs, exp, bw.last_range(d.p, 1))
        # one capped query over the sparse winners: its 8 winners (limit 7)
        # end near row 2300 of ~5400, far beyond one tile of NW*64 rows
        tile = (scan_t // 64) * 64
        s0 = bw.perf(d.p)["rows_scanned"]
        bw.bench_range(d.p, [(s, e, 0, 7)], 0)
        got = bw.last_range(d.p, 0)
        bw.check_records([(s, e, 0, 7)], bw.expected(d, [(s, e, 0, 7)],
                                                     d.p.current_rev()), got)
        scanned = bw.perf(d.p)["rows_scanned"] - s0
        # the delta run of the mixed case holds no winner, so it is read whole
        whole = p["delta_rows"] if residency == "base+delta-tombstones" else 0
        assert scanned - whole > tile, (scanned, whole, tile)   # a later tile ran
        assert scanned < span, (scanned, span)                  # the early exit worked
    finally:
        d.close()


def test_uncapped_scan_second_tile():
    """An unbounded scan tiles by NW*4096 rows: with 4 waves a span above
    16384 rows needs a second tile (the winner-count carry)."""
    d = bw.open_dual(KB_SCAN_T=256, KB_FLUSH_ROWS=1000000)
    try:
        keys, rev = build_versions(d, 2400, flush_after=True)
        s, e = TNS + b"/", TNS + b"0"
        p = bw.perf(d.p)
        assert p["base_rows"] == 2400 * 8 > 4 * 4096 and p["delta_rows"] == 0, p
        assert d.count(s, e)[2] == 2400
        d.list(s, e, 0, 0)
        # tombstones in the delta run thin the winners of both tiles
        dead = [k for i, k in enumerate(keys) if i % 5 == 2]
        for c0 in range(0, len(dead), 300):
            assert all(bw.dual_del(d, [(k, 0) for k in dead[c0:c0 + 300]]))
        assert d.count(s, e)[2] == 2400 - len(dead)
        d.list(s, e, 0, 0)
        bw.flush(d.p)
        assert d.count(s, e)[2] == 2400 - len(dead)
        d.list(s, e, 0, 0)
    finally:
        d.close()


# ---- d_lb_wave at the sizes where its 64-ary rounds change ------------------
SIZES = [2, 63, 64, 65, 66, 127, 128, 129, 4095, 4096, 4097, 4160, 4161]
WNS = b"/registry/pods/sweep"


@pytest.mark.parametrize("n", SIZES)
def test_search_size_sweep(n):
    d = bw.open_dual(KB_FLUSH_ROWS=1000000)
    try:
        u = n % 2 + 2 * min(3, n // 8)       # n = 2*creates + updates
        c = (n - u) // 2
        assert 2 * c + u == n and c >= 1
        keys = [WNS + b"/k-%05d" % i for i in range(c)]
        rev = {}
        for c0 in range(0, c, 1000):
            ops = [(k, 0, v(c0 + i, 10 + i % 30)) for i, k in enumerate(keys[c0:c0 + 1000])]
            for (k, _p, _v), r in zip(ops, bw.dual_txn(d, ops)):
                assert r
                rev[k] = r
        for j in range(u):                    # one more version each time
            k = keys[(j * 7) % c]
            (r,) = bw.dual_txn(d, [(k, rev[k], v(j, 21))])
            assert r
            rev[k] = r
        if c <= 65:
            probe = list(range(c))
        else:
            rng = np.random.default_rng(n)
            probe = sorted(set([0, 1, 2, c - 3, c - 2, c - 1]) |
                           {int(i) for i in rng.choice(c, 250, replace=False)})
        batch = None
        if n >= 4096:
            pick = np.random.default_rng(n + 1).choice(c, 1024, replace=False)
            batch = [(keys[int(i)], keys[int(i)] + b"0", 0, 0) for i in pick]
            exp = bw.expected(d, batch, d.p.current_rev())
            assert all(len(e) == 1 for e in exp)
        for where in ("delta", "base"):
            if where == "base":
                bw.flush(d.p)
            d.get(WNS + b"/a", 0)             # below the first key
            d.get(WNS + b"/z", 0)             # above the last key
            p = bw.perf(d.p)
            want = (0, n) if where == "delta" else (n, 0)
            assert (p["base_rows"], p["delta_rows"]) == want, (where, p)
            for i in probe:
                k = keys[i]
                assert d.get(k, 0)[2] is not None
                assert d.get(k + b"-", 0)[2] is None      # between two keys
                assert len(d.list(k, k + b"0", 0, 1).kvs) == 1
            if batch:
                assert bw.bench_range(d.p, batch, 1) == 1024
                bw.check_records(batch, exp, bw.last_range(d.p, 0))
                bw.check_records(batch, exp, bw.last_range(d.p, 1))
    finally:
        d.close()
