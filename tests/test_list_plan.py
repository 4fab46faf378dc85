"""CPU test of the pure host reply planner of kb_list_batch (lplan.h),
through the TEST-ONLY export kb_test_list_plan, against a Python model of the
reply layout: u32 n; n x 24-byte directory entry; then the sections in query
order. Needs no GPU."""
import ctypes as C
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OK, EINVALID, ENOBUF = 0, 5, 100
BIG = 1 << 40


def _lib():
    import kubebrain_amd
    return C.CDLL(kubebrain_amd.build())


def plan(status, host_len, dev_bytes, cap, arena=BIG, group=None):
    lib = _lib()
    n = len(status)
    m = max(n, 1)
    st = (C.c_int * m)(*status)
    hl = (C.c_longlong * m)(*host_len)
    db = (C.c_ulonglong * m)(*dev_bytes)
    gr = (C.c_int * m)(*group) if group is not None else None
    dlen = (C.c_ulonglong * m)()
    soff = (C.c_ulonglong * m)()
    rnd = (C.c_int * m)()
    span = (C.c_ulonglong * (2 * m))()
    nr = C.c_size_t(12345)
    req = C.c_size_t(12345)
    f = lib.kb_test_list_plan
    f.restype = C.c_int
    rc = f(st, hl, db, gr, C.c_size_t(n), C.c_size_t(cap), C.c_ulonglong(arena),
           dlen, soff, rnd, span, C.byref(nr), C.byref(req))
    if rc not in (OK, ENOBUF):
        return rc, None
    rounds = [(span[2 * r], span[2 * r + 1]) for r in range(nr.value)]
    return rc, {"len": list(dlen[:n]), "off": list(soff[:n]),
                "round": list(rnd[:n]), "rounds": rounds, "required": req.value}


def model(status, host_len, dev_bytes, arena=BIG, group=None):
    """Independent model: lengths, offsets, greedy rounds of whole queries."""
    n = len(status)
    off = 4 + 24 * n
    lens, offs, rnd, rounds = [], [], [], []
    cur_group = None
    for i in range(n):
        dev = status[i] == OK and host_len[i] < 0
        ln = 0 if status[i] != OK else (4 + dev_bytes[i] if dev else host_len[i])
        lens.append(ln)
        offs.append(off)
        if dev:
            g = group[i] if group is not None else 0
            if not rounds or g != cur_group or off + ln - rounds[-1][0] > arena:
                rounds.append([off, off])
                cur_group = g
            rounds[-1][1] = off + ln
            rnd.append(len(rounds) - 1)
        else:
            rnd.append(-1)
        off += ln
    return {"len": lens, "off": offs, "round": rnd,
            "rounds": [tuple(r) for r in rounds], "required": off}


def test_fixed_layout():
    st = [OK, EINVALID, OK, OK]
    hl = [-1, 0, 44, -1]
    db = [100, 0, 0, 0]
    rc, p = plan(st, hl, db, 1 << 20)
    assert rc == OK
    assert p["required"] == 4 + 4 * 24 + 104 + 44 + 4
    assert p["len"] == [104, 0, 44, 4]
    assert p["off"] == [100, 204, 204, 248]
    assert p["round"] == [0, -1, -1, 0]
    assert p["rounds"] == [(100, 252)]
    assert p == model(st, hl, db)


def test_enobuf_at_required_minus_one_and_tiny_caps():
    st, hl, db = [OK, OK], [-1, 9], [33, 0]
    rc, p = plan(st, hl, db, 1 << 20)
    assert rc == OK
    req = p["required"]
    assert req == 4 + 48 + 37 + 9
    for cap in (req - 1, 4 + 48 - 1, 4, 3, 0):
        rc2, p2 = plan(st, hl, db, cap)
        assert rc2 == ENOBUF, cap
        assert p2 == p, cap                      # same plan, same required size
    assert plan(st, hl, db, req)[0] == OK


def test_zero_queries():
    rc, p = plan([], [], [], 4)
    assert rc == OK and p["required"] == 4 and p["rounds"] == []
    for cap in (0, 3):
        rc, p = plan([], [], [], cap)
        assert rc == ENOBUF and p["required"] == 4


def test_all_error_batch():
    # a non-OK status has len 0 whatever host_len / dev_bytes say
    st = [EINVALID, 12, 11, 4]
    rc, p = plan(st, [0, -1, 99, 4], [7, 7, 7, 7], 1 << 20)
    assert rc == OK
    assert p["len"] == [0, 0, 0, 0]
    assert p["required"] == 4 + 4 * 24
    assert p["off"] == [100] * 4
    assert p["round"] == [-1] * 4 and p["rounds"] == []
    assert plan(st, [0, -1, 99, 4], [7, 7, 7, 7], 4 + 4 * 24 - 1)[0] == ENOBUF


def test_rounds_and_groups():
    st = [OK] * 6
    hl = [-1, -1, 500, -1, -1, -1]
    db = [96, 96, 0, 96, 96, 96]              # device sections of 100 bytes
    # arena of 200: two sections per round; the host section is a hole that
    # pushes query 3 out of round 0's span
    rc, p = plan(st, hl, db, 1 << 20, arena=200)
    assert rc == OK
    assert p["round"] == [0, 0, -1, 1, 1, 2]
    assert p == model(st, hl, db, arena=200)
    # sub-batch boundaries split rounds even when the arena has room
    rc, p = plan(st, hl, db, 1 << 20, arena=BIG, group=[0, 0, 0, 0, 1, 1])
    assert p["round"] == [0, 0, -1, 0, 1, 1]
    assert p == model(st, hl, db, group=[0, 0, 0, 0, 1, 1])
    # a device section larger than the arena is not the planner's to place
    assert plan(st, hl, db, 1 << 20, arena=99)[0] == EINVALID
    # an OK host section is at least its u32 count
    assert plan([OK], [3], [0], 1 << 20)[0] == EINVALID
    assert plan([OK], [4], [0], 1 << 20)[0] == OK


def test_random_against_model():
    rng = random.Random(20)
    for _ in range(300):
        n = rng.randrange(0, 50)
        arena = rng.randrange(64, 5000)
        st = [rng.choice([OK, OK, OK, EINVALID, 4]) for _ in range(n)]
        hl = [rng.choice([-1, -1, rng.randrange(4, 3000)]) for _ in range(n)]
        db = [rng.choice([0, rng.randrange(0, arena - 3)]) for _ in range(n)]
        g, group = 0, []
        for _i in range(n):
            g += rng.random() < 0.1
            group.append(g)
        want = model(st, hl, db, arena, group)
        rc, got = plan(st, hl, db, want["required"], arena, group)
        assert rc == OK and got == want
        rc, got = plan(st, hl, db, want["required"] - 1, arena, group)
        assert rc == ENOBUF and got == want
        for lo, hi in want["rounds"]:
            assert 0 < hi - lo <= arena
