"""Test helper for the batched bench entry points (kb_bench_range,
kb_bench_step, kb_bench_txn, kb_bench_del) and the kb_test_last_range hook:
packs their inputs, reads the records of the last Range batch back and
parses that wire. Pure Python over ctypes; parse_wire needs no GPU."""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import os
import struct

import numpy as np

ENOBUF = 100
HDR = 32  # per-query directory entry: i64 written, total, bytes; i32 ovf; i32 0


def pad16(n: int) -> int:
    return (n + 15) & ~15


# ---- packing (parseBenchQueries / BenchTxn / BenchDel layouts) -------------
def pack_queries(qs) -> bytes:
    """qs = [(start, end, rev, limit)] -> n x {u32 slen; u32 elen; u64 rev;
    u64 limit; start; end}."""
    parts = []
    for s, e, rev, limit in qs:
        parts.append(struct.pack("<IIQQ", len(s), len(e), rev, limit))
        parts.append(s)
        parts.append(e)
    return b"".join(parts)


def pack_txns(ops) -> bytes:
    """ops = [(key, prev_rev, val)] -> n x {u32 klen; u64 prev; u32 vlen; key; val}."""
    parts = []
    for k, prev, v in ops:
        parts.append(struct.pack("<IQI", len(k), prev, len(v)))
        parts.append(k)
        parts.append(v)
    return b"".join(parts)


def pack_dels(ops) -> bytes:
    """ops = [(key, prev_rev)] -> n x {u32 klen; u64 prev; key}."""
    parts = []
    for k, prev in ops:
        parts.append(struct.pack("<IQ", len(k), prev))
        parts.append(k)
    return b"".join(parts)


# ---- calls on the product store -------------------------------------------
def _err(store) -> str:
    buf = C.create_string_buffer(512)
    store.lib.kb_last_error(buf, C.c_size_t(512))
    return buf.value.decode(errors="replace")


def bench_range(store, qs, mode: int) -> int:
    tot = C.c_ulonglong()
    secs = C.c_double()
    rc = store._f("bench_range")(C.c_void_p(store.h), pack_queries(qs),
                                 C.c_size_t(len(qs)), C.c_int(mode),
                                 C.byref(tot), C.byref(secs))
    assert rc == 0, (rc, _err(store))
    return tot.value


def bench_step(store, qs, ops, mode: int):
    """-> (total, [new revision or 0 per op])."""
    tot = C.c_ulonglong()
    secs = C.c_double()
    out = np.zeros(max(len(ops), 1), dtype=np.uint64)
    rc = store._f("bench_step")(C.c_void_p(store.h), pack_queries(qs),
                                C.c_size_t(len(qs)), pack_txns(ops),
                                C.c_size_t(len(ops)), C.c_int(mode),
                                out.ctypes.data_as(C.POINTER(C.c_uint64)),
                                C.byref(tot), C.byref(secs))
    assert rc == 0, (rc, _err(store))
    return tot.value, [int(x) for x in out[:len(ops)]]


def bench_txn(store, ops):
    out = np.zeros(max(len(ops), 1), dtype=np.uint64)
    rc = store._f("bench_txn")(C.c_void_p(store.h), pack_txns(ops),
                               C.c_size_t(len(ops)),
                               out.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == 0, (rc, _err(store))
    return [int(x) for x in out[:len(ops)]]


def bench_del(store, ops):
    out = np.zeros(max(len(ops), 1), dtype=np.uint64)
    rc = store._f("bench_del")(C.c_void_p(store.h), pack_dels(ops),
                               C.c_size_t(len(ops)),
                               out.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == 0, (rc, _err(store))
    return [int(x) for x in out[:len(ops)]]


def sync(store):
    rc = store._f("sync")(C.c_void_p(store.h))
    assert rc == 0, (rc, _err(store))


def flush(store):
    rc = store._f("flush")(C.c_void_p(store.h))
    assert rc == 0, (rc, _err(store))


def perf(store) -> dict:
    buf = C.create_string_buffer(8192)
    rc = store._f("perf_json")(C.c_void_p(store.h), buf, C.c_size_t(8192))
    assert rc == 0, rc
    return json.loads(buf.value.decode())


def last_range_raw(store, src: int, first_cap: int = 1 << 16) -> bytes:
    """kb_test_last_range with grow-and-retry on KB_ENOBUF."""
    f = store._f("test_last_range")
    cap = first_cap
    out_len = C.c_size_t()
    for _ in range(3):
        buf = C.create_string_buffer(cap)
        rc = f(C.c_void_p(store.h), C.c_int(src), buf, C.c_size_t(cap),
               C.byref(out_len))
        if rc != ENOBUF:
            break
        assert out_len.value > cap, (out_len.value, cap)
        cap = out_len.value
    assert rc == 0, (rc, _err(store))
    return C.string_at(buf, out_len.value)


def last_range(store, src: int):
    return parse_wire(last_range_raw(store, src))


# ---- the wire --------------------------------------------------------------
def parse_wire(raw: bytes):
    """-> [(written, total, bytes, overflow, [(rev, key, val)])] per query.
    Raises ValueError on a truncated or inconsistent buffer. Padding bytes
    are skipped, never inspected (the device arena is not zeroed)."""
    if len(raw) < 4:
        raise ValueError("wire shorter than its count")
    (nq,) = struct.unpack_from("<I", raw, 0)
    if len(raw) < 4 + nq * HDR:
        raise ValueError("wire shorter than its directory")
    off = 4 + nq * HDR
    res = []
    for q in range(nq):
        written, total, nbytes, ovf, zero = struct.unpack_from(
            "<qqqii", raw, 4 + q * HDR)
        if written < 0 or total < 0 or nbytes < 0 or ovf not in (0, 1) or zero:
            raise ValueError(f"query {q}: bad directory entry "
                             f"{(written, total, nbytes, ovf, zero)}")
        recs = []
        if not ovf:
            end = off + nbytes
            if end > len(raw):
                raise ValueError(f"query {q}: records run past the buffer")
            for j in range(written):
                if off + 16 > end:
                    raise ValueError(f"query {q} record {j}: header past the "
                                     "query's bytes")
                rev, klen, vlen = struct.unpack_from("<QII", raw, off)
                size = 16 + pad16(klen) + pad16(vlen)
                if off + size > end:
                    raise ValueError(f"query {q} record {j}: klen={klen} "
                                     f"vlen={vlen} past the query's bytes")
                key = raw[off + 16:off + 16 + klen]
                voff = off + 16 + pad16(klen)
                recs.append((rev, key, raw[voff:voff + vlen]))
                off += size
            if off != end:
                raise ValueError(f"query {q}: bytes={nbytes} but its {written} "
                                 f"records take {nbytes - (end - off)}")
        res.append((written, total, nbytes, bool(ovf), recs))
    if off != len(raw):
        raise ValueError(f"{len(raw) - off} trailing bytes")
    return res


def build_wire(queries) -> bytes:
    """Inverse of parse_wire for hand-built fixtures: queries =
    [(written, total, overflow, [(rev, key, val)])]; padding is 0xA5 so a
    parser that reads it shows up."""
    head, body = [struct.pack("<I", len(queries))], []
    for written, total, ovf, recs in queries:
        blob = b""
        for rev, key, val in recs:
            blob += struct.pack("<QII", rev, len(key), len(val))
            blob += key + b"\xa5" * (pad16(len(key)) - len(key))
            blob += val + b"\xa5" * (pad16(len(val)) - len(val))
        head.append(struct.pack("<qqqii", written, total, len(blob),
                                1 if ovf else 0, 0))
        if not ovf:
            body.append(blob)
    return b"".join(head + body)


# ---- stores under their own knobs -------------------------------------------
# device allocations sized for stores of at most ~20k rows, so that opening
# one store per test case stays cheap
SMALL = {"KB_MAX_ROWS": str(1 << 17), "KB_HEAP_BYTES": str(64 << 20),
         "KB_SPILL_BYTES": str(16 << 20)}


@contextlib.contextmanager
def env(**kw):
    """Set environment knobs (read by kb_new) for the duration of the block."""
    new = dict(SMALL)
    new.update({k: str(v) for k, v in kw.items()})
    old = {k: os.environ.get(k) for k in new}
    os.environ.update(new)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def open_dual(**kw):
    """A parity.Dual whose product store is created under the given knobs."""
    import parity
    with env(**kw):
        return parity.Dual()


# ---- product batch + oracle serial replay ---------------------------------
def dual_txn(d, ops):
    """One kb_bench_txn batch (unique keys) on the product, the same ops
    through the oracle's serial Update; per-op results must agree.
    -> [new revision or 0]."""
    revs = bench_txn(d.p, ops)
    for (k, prev, v), nr in zip(ops, revs):
        ro = d.o.update(k, v, prev)
        assert (ro.header_revision if ro.succeeded else 0) == nr, (k, prev, ro, nr)
    return revs


def dual_del(d, ops):
    revs = bench_del(d.p, ops)
    for (k, prev), nr in zip(ops, revs):
        ro = d.o.delete(k, prev)
        assert (ro.header_revision if ro.succeeded else 0) == nr, (k, prev, ro, nr)
    return revs


def expected(d, qs, cur, cache=None):
    """Oracle winners per query: list(s, e, rev or cur, 0).kvs as
    [(rev, key, val)]. cache (dict) shares results between tests."""
    out = []
    for s, e, rev, _limit in qs:
        key = (s, e, rev or cur)
        if cache is not None and key in cache:
            out.append(cache[key])
            continue
        lo = d.o.list(s, e, rev or cur, 0)
        assert lo.status == 0, (s, e, rev, lo.status)
        kvs = [(kv.revision, kv.key, kv.value) for kv in lo.kvs]
        if cache is not None:
            cache[key] = kvs
        out.append(kvs)
    return out


def check_records(qs, exp, got, keys_only=False, allow_overflow=()):
    """got = parse_wire output for the batch qs; exp = expected(...)."""
    assert len(got) == len(qs), (len(got), len(qs))
    for i, ((s, e, rev, limit), ex, (written, total, nbytes, ovf, recs)) in \
            enumerate(zip(qs, exp, got)):
        ctx = (i, s, e, rev, limit)
        if i in allow_overflow:
            assert ovf and not recs, ctx
            continue
        assert not ovf, ctx
        want_n = min(len(ex), limit + 1) if limit else len(ex)
        assert written == want_n, (ctx, written, want_n, len(ex))
        if limit == 0:
            assert total == len(ex), (ctx, total, len(ex))
        assert len(recs) == written, ctx
        want = ex[:written]
        if keys_only:
            want = [(r, k, b"") for r, k, _ in want]
        if recs != want:
            for j, (a, b) in enumerate(zip(recs, want)):
                assert a == b, (ctx, j, a[:2], b[:2], len(a[2]), len(b[2]))
        assert nbytes == sum(16 + pad16(len(k)) + pad16(len(v))
                             for _, k, v in want), ctx
