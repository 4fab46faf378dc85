"""CPU tests for the pure host reply planner of kb_watch_poll_batch
(kb_test_wpoll_plan -> wpoll.h Plan): the directory, the per-ref destination
offsets, the required size and the ENOBUF decision, checked against a
few-line Python restatement of the reply layout

    u32 n; n x { i32 status; u32 len; len bytes }

No GPU needed: the symbol is pure host code in libkbslab.so.
"""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OK, EINVALID, DROPPED, ENOBUF = 0, 5, 10, 100


@pytest.fixture(scope="module")
def lib():
    from kubebrain_amd import build
    return C.CDLL(build())


def plan(lib, refs, watchers, cap):
    """refs: [(bytes, count, widx)]; watchers: [(status, host_len)] with
    host_len < 0 = device path."""
    nr, n = len(refs), len(watchers)
    rb = (C.c_ulonglong * max(nr, 1))(*[r[0] for r in refs])
    rc_ = (C.c_uint * max(nr, 1))(*[r[1] for r in refs])
    rw = (C.c_int * max(nr, 1))(*[r[2] for r in refs])
    st = (C.c_int * max(n, 1))(*[w[0] for w in watchers])
    hl = (C.c_longlong * max(n, 1))(*[w[1] for w in watchers])
    dl = (C.c_uint * max(n, 1))()
    dc = (C.c_uint * max(n, 1))()
    so = (C.c_ulonglong * max(n, 1))()
    ro = (C.c_ulonglong * max(nr, 1))()
    req = C.c_size_t(0xdead)
    rc = lib.kb_test_wpoll_plan(rb, rc_, rw, C.c_size_t(nr), st, hl,
                                C.c_size_t(n), C.c_size_t(cap), dl, dc, so, ro,
                                C.byref(req))
    return (rc, list(dl)[:n], list(dc)[:n], list(so)[:n], list(ro)[:nr],
            req.value)


def model(refs, watchers, cap):
    off = 4
    lens, counts, secs, roffs = [], [], [], [None] * len(refs)
    for i, (st, hl) in enumerate(watchers):
        off += 8
        secs.append(off)
        if st != OK:
            ln, cnt = 0, 0
        elif hl >= 0:
            ln, cnt = hl, 0
        else:
            ln, cnt = 4, 0
            for r, (b, c, w) in enumerate(refs):
                if w == i:
                    roffs[r] = off + ln
                    ln += b
                    cnt += c
        lens.append(ln)
        counts.append(cnt)
        off += ln
    return (OK if off <= cap else ENOBUF), lens, counts, secs, roffs, off


MIXED_REFS = [(580, 1, 0), (1160, 2, 0), (33, 1, 3), (5000, 9, 5), (1, 1, 5),
              (17, 1, 5)]
MIXED_WATCHERS = [(OK, -1), (DROPPED, 0), (OK, 4 + 28 + 40 + 7), (OK, -1),
                  (OK, 4), (OK, -1), (DROPPED, 0)]


def test_mixed_device_host_dropped(lib):
    got = plan(lib, MIXED_REFS, MIXED_WATCHERS, 1 << 20)
    want = model(MIXED_REFS, MIXED_WATCHERS, 1 << 20)
    assert got == want
    rc, lens, counts, secs, roffs, req = got
    assert rc == OK
    assert lens[1] == lens[6] == 0          # dropped: len 0
    assert lens[0] == 4 + 580 + 1160 and counts[0] == 3
    assert counts[5] == 11
    # records of one watcher are contiguous, in ref order, after its count
    assert roffs[0] == secs[0] + 4 and roffs[1] == roffs[0] + 580
    assert roffs[4] == roffs[3] + 5000 and roffs[5] == roffs[4] + 1
    assert req == 4 + 8 * len(MIXED_WATCHERS) + sum(lens)


def test_zero_event_watchers(lib):
    # a device-path watcher with no refs and a host-path one with no events:
    # both sections are a bare u32 0, len 4
    ws = [(OK, -1), (OK, 4), (OK, -1)]
    refs = [(100, 1, 2)]
    got = plan(lib, refs, ws, 4096)
    assert got == model(refs, ws, 4096)
    assert got[1] == [4, 4, 104] and got[2] == [0, 0, 1]


def test_cap_exact_and_one_short(lib):
    _, _, _, _, _, req = model(MIXED_REFS, MIXED_WATCHERS, 0)
    got = plan(lib, MIXED_REFS, MIXED_WATCHERS, req)
    assert got[0] == OK and got[5] == req
    got = plan(lib, MIXED_REFS, MIXED_WATCHERS, req - 1)
    assert got[0] == ENOBUF and got[5] == req
    # the plan itself does not depend on cap
    assert got[1:] == plan(lib, MIXED_REFS, MIXED_WATCHERS, req)[1:]


@pytest.mark.parametrize("cap", [0, 3])
def test_cap_below_header(lib, cap):
    got = plan(lib, MIXED_REFS, MIXED_WATCHERS, cap)
    assert got[0] == ENOBUF
    assert got[5] == model(MIXED_REFS, MIXED_WATCHERS, cap)[5]
    assert plan(lib, [], [], cap) == (ENOBUF, [], [], [], [], 4)


def test_n_zero(lib):
    assert plan(lib, [], [], 4) == (OK, [], [], [], [], 4)
    assert plan(lib, [], [], 1 << 20) == (OK, [], [], [], [], 4)


def test_rejects_misordered_refs(lib):
    # a ref naming a host-path, a dropped or an out-of-range watcher, or refs
    # out of watcher order, cannot be laid out: EINVALID
    ws = [(OK, -1), (OK, 32), (DROPPED, 0), (OK, -1)]
    assert plan(lib, [(8, 1, 1)], ws, 4096)[0] == EINVALID
    assert plan(lib, [(8, 1, 2)], ws, 4096)[0] == EINVALID
    assert plan(lib, [(8, 1, 4)], ws, 4096)[0] == EINVALID
    assert plan(lib, [(8, 1, 3), (8, 1, 0)], ws, 4096)[0] == EINVALID
    assert plan(lib, [(8, 1, 0), (8, 1, 3)], ws, 4096)[0] == OK
