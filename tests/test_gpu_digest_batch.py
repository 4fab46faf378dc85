"""GPU tests for kb_digest_batch: per range the count, key bytes, value bytes
and record-hash sum of the kvs an unbounded List returns, reduced across the
chip by k_digest_plan / k_digest_tiles.

Reference for every entry: the ORACLE's unbounded list(start, end, rev) hashed
by the plain Python implementation in tests/test_digest_record.py. The whole
expected reply (u32 n; n x {i32 status; i32 0; u64 header_rev; u64 count; u64
key_bytes; u64 value_bytes; u64 hash}) is serialized in Python and compared
with the reply bytes as a whole. Every case also asserts from kb_perf_json
that the digest kernels served every valid query and that the scan, gather
and list-emit kernels stayed idle, so a fallback through List cannot pass.
"""
import ctypes as C
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import benchwire as bw
import parity
import test_digest_record as tdr
import test_gpu_bench_records as tbr
from kbclient import BADKEY, COMPACTED, ENOBUF, INVALID_ARG, KEYTOOLONG, OK

pytestmark = pytest.mark.gpu

parity.small_env()

DEFAULT_TILE = 1024
EDGE = b"/registry/pods/ns-edge"
EDGE_VLENS = [0, 1, 15, 16, 17, 255, 256, 257, 4097]   # group-step and tail-mask edges
IDLE = ("scan_launches", "gather_launches", "list_emit_launches")
WHOLE = (b"/registry/", b"/registry0")
_memo = {}


def rec_hash(rev, key, val, konly):
    k = (rev, key, b"" if konly else val)
    if k not in _memo:
        _memo[k] = tdr.record(rev, key, val, konly)
    return _memo[k]


def bound_status(b):
    """validateBound (include/kb_slab.h): at most 4096 bytes, no byte <= 0x24
    except trailing 0x00."""
    if len(b) > 4096:
        return KEYTOOLONG
    return BADKEY if any(c <= 0x24 for c in b.rstrip(b"\x00")) else OK


def oracle_entry(d, q, konly):
    s, e, rev, _limit = q
    hdr = d.o.current_rev()
    bad = bound_status(s) or bound_status(e)
    if bad or s >= e:
        return (bad, hdr, 0, 0, 0, 0)
    lo = d.o.list(s, e, rev or hdr, 0)
    if lo.status != OK:
        return (lo.status, hdr, 0, 0, 0, 0)
    kvs = lo.kvs
    return (OK, hdr, len(kvs), sum(len(kv.key) for kv in kvs),
            sum(len(kv.value) for kv in kvs),
            sum(rec_hash(kv.revision, kv.key, kv.value, konly) for kv in kvs) & tdr.M)


def check_batch(d, qs, konly, tile=DEFAULT_TILE):
    exp = [oracle_entry(d, q, konly) for q in qs]
    nvalid = sum(e[0] == OK for e in exp)
    before = bw.perf(d.p)
    rc, res, raw = d.p.digest_batch(qs, keys_only=konly)
    after = bw.perf(d.p)
    assert rc == OK, (rc, bw._err(d.p))
    for i, (a, b) in enumerate(zip(res, exp)):        # say where, then the whole
        assert a == b, (i, qs[i][0][-30:], qs[i][1][-30:], qs[i][2], a, b)
    assert raw == struct.pack("<I", len(exp)) + b"".join(
        struct.pack("<iiQQQQQ", e[0], 0, *e[1:]) for e in exp)
    delta = {k: after[k] - before[k] for k in after if isinstance(after[k], int)}
    assert delta["digest_batch_calls"] == 1 and delta["digest_batch_q"] == nvalid, delta
    assert all(delta[k] == 0 for k in IDLE), delta
    if nvalid:
        assert delta["digest_batch_launches"] >= 1, delta
    rows, tiles = delta["digest_batch_rows"], delta["digest_batch_tiles"]
    assert -(-rows // tile) <= tiles <= rows // tile + 2 * nvalid, delta
    assert delta["digest_batch_kvs"] == sum(e[2] for e in exp)
    assert delta["digest_batch_bytes"] == sum(e[3] + (0 if konly else e[4]) for e in exp)
    return exp, delta


@pytest.fixture(scope="module", params=[(64, False), (64, True), (None, False), (None, True)],
                ids=["tile64-delta", "tile64-flushed", "default-delta", "default-flushed"])
def world(request):
    """The bench-records fixture store (~3000 rows over base and delta, 1..5
    versions per key, tombstones, recreated keys, 96/97/300-byte keys) plus
    one namespace of values at the group-step and tail-mask edges; flushed =
    after kb_flush (delta empty, shadow idle)."""
    tile, flushed = request.param
    d = bw.open_dual(**({"KB_DIGEST_TILE": tile} if tile else {}))
    try:
        info = tbr.build(d)
        ops = [(EDGE + b"/obj-%02d" % i, 0, tbr.val(40 + i, n)) for i, n in enumerate(EDGE_VLENS)]
        assert all(bw.dual_txn(d, ops))
        if flushed:
            bw.flush(d.p)
        d.count(*WHOLE)                                   # device state current
        p = bw.perf(d.p)
        assert (p["delta_rows"] == 0) == flushed and p["base_rows"] > 0, p
        yield d, info, tile or DEFAULT_TILE
    finally:
        d.close()


@pytest.mark.parametrize("konly", [False, True], ids=["full", "keys_only"])
def test_digest_matches_oracle(world, konly):
    d, info, tile = world
    one = tbr.key(tbr.NS[2], 17)
    ranges = [WHOLE, (EDGE + b"/", EDGE + b"0"), (tbr.FAT + b"/", tbr.FAT + b"0"),
              (tbr.P96, tbr.P96 + b"c"), (one, one + b"0"),            # long keys; one key
              (one + b"-", one + b"-z"), (tbr.NS[1] + b"0", tbr.NS[1] + b"/")]  # empty; start >= end
    ranges += [(ns + b"/", ns + b"0") for ns in tbr.NS]
    h = info["hist"]
    qs = [(s, e, r, 0) for r in (0, h[1], h[0]) for s, e in ranges]
    qs += [(b"/registry/\x01x", b"/registry0", 0, 0),                  # bad byte
           (b"/registry/", b"/registry/" + b"k" * 4200, h[1], 0)]      # over-long
    exp, delta = check_batch(d, qs, konly, tile)
    assert [e[0] for e in exp[-2:]] == [BADKEY, KEYTOOLONG]
    by = dict(zip(qs, exp))
    assert by[WHOLE + (0, 0)][2] > 1000 and by[ranges[1] + (0, 0)][2:5] == (
        9, 9 * len(EDGE + b"/obj-00"), sum(EDGE_VLENS))
    assert by[ranges[3] + (0, 0)][2] >= 2 and by[ranges[4] + (0, 0)][2] <= 1
    assert by[ranges[5] + (0, 0)][2:] == (0, 0, 0, 0) == by[ranges[6] + (h[1], 0)][2:]
    assert len({e[5] for e in exp if e[2]}) > 15                       # hashes differ
    if tile == 64:
        assert delta["digest_batch_tiles"] > 100, delta


def test_compacted_revision():
    ns = b"/registry/cp"
    d = bw.open_dual(KB_FLUSH_ROWS=100000)
    try:
        keys = [ns + b"/k-%02d" % i for i in range(30)]
        rev = {k: d.create(k, tbr.val(i, 20 + i)).header_revision for i, k in enumerate(keys)}
        for i, k in enumerate(keys[::3]):
            rev[k] = d.update(k, tbr.val(100 + i, 33), rev[k]).header_revision
        mid = rev[keys[18]]
        for k in keys[1::5]:
            assert d.delete(k, rev[k]).succeeded
        assert d.compact(mid)[0] == OK
        rng_ = (ns + b"/", ns + b"0")
        qs = [rng_ + (0, 0), rng_ + (mid - 1, 0), rng_ + (mid, 0), rng_ + (1, 0),
              rng_ + (mid + 2, 0)]
        for konly in (False, True):
            exp, delta = check_batch(d, qs, konly)
            assert [e[0] for e in exp] == [OK, COMPACTED, OK, COMPACTED, OK]
            assert exp[0][2] == 30 - len(keys[1::5]) and delta["digest_batch_q"] == 3
    finally:
        d.close()


def raw_call(store, qs, flags, cap, slack=64):
    """kb_digest_batch with an exact cap and a canary behind it.
    -> (rc, out_len, total_kvs, bytes [0, cap), canary intact?)."""
    buf = C.create_string_buffer(b"\xc3" * (cap + slack), cap + slack)
    out_len, total = C.c_size_t(0), C.c_ulonglong(0)
    rc = store._f("digest_batch")(C.c_void_p(store.h), store.encode_queries(qs),
                                  C.c_size_t(len(qs)), C.c_int(flags), buf,
                                  C.c_size_t(cap), C.byref(out_len), C.byref(total))
    mem = C.string_at(buf, cap + slack)
    return rc, out_len.value, total.value, mem[:cap], mem[cap:] == b"\xc3" * slack


def test_call_shape():
    ns = b"/registry/cs"
    max_q = 8
    d = bw.open_dual(KB_MAX_Q=max_q)
    try:
        keys = [ns + b"/k-%02d" % i for i in range(25)]
        for i, k in enumerate(keys):
            d.create(k, tbr.val(i, 3 * i))
        # n = 0
        assert raw_call(d.p, [], 0, 4) == (OK, 4, 0, b"\x00\x00\x00\x00", True)
        check_batch(d, [], False)
        # n = 2 KB_MAX_Q + 3: three launches, entries in query order
        n = 2 * max_q + 3
        qs = [(keys[i], keys[i + 1 + i % 6], 0, 0) for i in range(n)]
        qs[4] = (b"/registry/\x03", keys[0], 0, 0)        # one bad query inside
        exp, delta = check_batch(d, qs, False)
        assert delta["digest_batch_launches"] == 3 and delta["digest_batch_q"] == n - 1
        assert [e[2] for e in exp] == [0 if i == 4 else 1 + i % 6 for i in range(n)]
        # a bad flag: nothing written, no launch
        need = 4 + 48 * n
        for flags, cap, want in [(2, 256, (INVALID_ARG, 0)), (-1, 256, (INVALID_ARG, 0)),
                                 (0, need - 1, (ENOBUF, need)), (1, 3, (ENOBUF, need))]:
            before = bw.perf(d.p)
            rc, ln, tot, out, ok = raw_call(d.p, qs, flags, cap)
            assert (rc, ln) == want and tot == 0 and ok and out == b"\xc3" * cap, (flags, cap)
            assert bw.perf(d.p)["digest_batch_launches"] == before["digest_batch_launches"]
        rc, ln, tot, out, ok = raw_call(d.p, qs, 0, need)   # exactly the required size
        assert (rc, ln, ok) == (OK, need, True) and tot == sum(e[2] for e in exp)
        assert out == d.p.digest_batch(qs)[2]
        # the last Range batch's records survive the call byte for byte
        rq = [(keys[0], keys[20], 0, 0), (keys[3], keys[9], 0, 2)]
        assert bw.bench_range(d.p, rq, 0) == 20 + 2
        raw0 = bw.last_range_raw(d.p, 0)
        check_batch(d, qs, True)
        assert bw.last_range_raw(d.p, 0) == raw0
    finally:
        d.close()
