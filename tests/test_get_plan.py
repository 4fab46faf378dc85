"""CPU test of the pure host reply planner of kb_get_batch (gplan.h), through
the TEST-ONLY export kb_test_get_plan, against a Python model of the reply
layout (u32 n; n x 32-byte directory entry; then the values of the has_kv
entries in query order) and of the emit rounds. Needs no GPU."""
import ctypes as C
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OK, EINVALID, ENOBUF = 0, 5, 100
BIG = 1 << 40
NONE, HOST = -1, -2


def _lib():
    import kubebrain_amd
    return C.CDLL(kubebrain_amd.build())


def plan(has_kv, vlen, cap, arena=BIG, max_q=1024):
    lib = _lib()
    n = len(has_kv)
    m = max(n, 1)
    hk = (C.c_int * m)(*has_kv)
    vl = (C.c_ulonglong * m)(*vlen)
    voff = (C.c_ulonglong * m)()
    rnd = (C.c_int * m)()
    span = (C.c_ulonglong * (2 * m))()
    nr, nh, req = C.c_size_t(12345), C.c_size_t(12345), C.c_size_t(12345)
    found = C.c_ulonglong(12345)
    f = lib.kb_test_get_plan
    f.restype = C.c_int
    rc = f(hk, vl, C.c_size_t(n), C.c_size_t(max_q), C.c_size_t(cap),
           C.c_ulonglong(arena), voff, rnd, span, C.byref(nr), C.byref(nh),
           C.byref(req), C.byref(found))
    if rc not in (OK, ENOBUF):
        return rc, None
    rounds = [(span[2 * r], span[2 * r + 1]) for r in range(nr.value)]
    return rc, {"off": list(voff[:n]), "round": list(rnd[:n]), "rounds": rounds,
                "n_host": nh.value, "required": req.value, "found": found.value}


def model(has_kv, vlen, arena=BIG, max_q=1024):
    """Independent model. A round = a maximal run of consecutive queries of
    one sub-batch (i // max_q) whose values fit the arena together; a value
    larger than the arena is host path and ends the run."""
    n = len(has_kv)
    off = 4 + 32 * n
    offs, rnd, rounds = [], [], []
    fill = None                      # bytes in the open round, None = closed
    for i in range(n):
        if i % max_q == 0:
            fill = None
        offs.append(off)
        ln = vlen[i] if has_kv[i] else 0
        if ln == 0:
            rnd.append(NONE)
            continue
        off += ln
        if ln > arena:
            rnd.append(HOST)
            fill = None
            continue
        if fill is None or fill + ln > arena:
            rounds.append([i, i])
            fill = 0
        fill += ln
        rounds[-1][1] = i + 1
        rnd.append(len(rounds) - 1)
    return {"off": offs, "round": rnd, "rounds": [tuple(r) for r in rounds],
            "n_host": rnd.count(HOST), "required": off, "found": sum(map(bool, has_kv))}


def test_fixed_layout():
    hk, vl = [1, 0, 1, 1], [100, 0, 0, 60]
    rc, p = plan(hk, vl, 1 << 20)
    assert rc == OK
    assert p["required"] == 4 + 4 * 32 + 160
    assert p["off"] == [132, 232, 232, 232]
    assert p["round"] == [0, NONE, NONE, 0]
    assert p["rounds"] == [(0, 4)]
    assert (p["found"], p["n_host"]) == (3, 0)
    assert p == model(hk, vl)


def test_zero_queries_and_all_not_found():
    rc, p = plan([], [], 4)
    assert rc == OK and p["required"] == 4 and p["rounds"] == [] and p["found"] == 0
    for cap in (0, 3):
        rc, p = plan([], [], cap)
        assert rc == ENOBUF and p["required"] == 4
    rc, p = plan([0] * 5, [0] * 5, 4 + 160)
    assert rc == OK
    assert p == model([0] * 5, [0] * 5)
    assert p["required"] == 164 and p["round"] == [NONE] * 5 and p["found"] == 0
    assert plan([0] * 5, [0] * 5, 163)[0] == ENOBUF


def test_enobuf_at_required_minus_one_and_tiny_caps():
    hk, vl = [1, 1, 0], [33, 9, 0]
    rc, p = plan(hk, vl, 1 << 20)
    assert rc == OK
    req = p["required"]
    assert req == 4 + 96 + 42
    for cap in (req - 1, 4 + 96 - 1, 4, 3, 0):
        rc2, p2 = plan(hk, vl, cap)
        assert rc2 == ENOBUF, cap
        assert p2 == p, cap                      # same plan, same required size
    assert plan(hk, vl, req)[0] == OK


def test_one_two_and_more_rounds():
    hk, vl = [1] * 6, [100] * 6
    for arena, want in ((600, 1), (BIG, 1), (300, 2), (599, 2), (200, 3),
                        (199, 6), (100, 6)):
        rc, p = plan(hk, vl, 1 << 20, arena=arena)
        assert rc == OK and len(p["rounds"]) == want, (arena, p)
        assert p == model(hk, vl, arena)
        assert p["n_host"] == 0
    # sub-batch boundaries split rounds even when the arena has room
    rc, p = plan(hk, vl, 1 << 20, max_q=4)
    assert p["round"] == [0, 0, 0, 0, 1, 1] and p["rounds"] == [(0, 4), (4, 6)]
    # queries without bytes lie inside a round's range but in no round
    hk2, vl2 = [0, 1, 1, 0, 1, 0], [0, 50, 0, 0, 50, 0]
    rc, p = plan(hk2, vl2, 1 << 20, arena=100)
    assert p["round"] == [NONE, 0, NONE, NONE, 0, NONE] and p["rounds"] == [(1, 5)]
    assert p["found"] == 3 and p == model(hk2, vl2, 100)


def test_value_equal_to_the_arena_and_one_byte_larger():
    hk = [1, 1, 1]
    rc, p = plan(hk, [10, 500, 10], 1 << 20, arena=500)
    assert rc == OK and p["n_host"] == 0
    assert p["round"] == [0, 1, 2] and p["rounds"] == [(0, 1), (1, 2), (2, 3)]
    rc, p = plan(hk, [10, 501, 10], 1 << 20, arena=500)
    assert rc == OK and p["n_host"] == 1
    assert p["round"] == [0, HOST, 1] and p["rounds"] == [(0, 1), (2, 3)]
    assert p["off"] == [100, 110, 611] and p["required"] == 621
    assert p == model(hk, [10, 501, 10], 500)


def test_host_path_first_last_and_between_rounds():
    for vl, want_round, want_rounds in (
            ([900, 10, 20], [HOST, 0, 0], [(1, 3)]),
            ([10, 20, 900], [0, 0, HOST], [(0, 2)]),
            ([60, 60, 900, 60, 60], [0, 1, HOST, 2, 3],
             [(0, 1), (1, 2), (3, 4), (4, 5)]),
            ([30, 30, 900, 30, 30], [0, 0, HOST, 1, 1], [(0, 2), (3, 5)]),
            ([900, 900], [HOST, HOST], [])):
        hk = [1] * len(vl)
        rc, p = plan(hk, vl, 1 << 20, arena=100)
        assert rc == OK
        assert p["round"] == want_round and p["rounds"] == want_rounds, vl
        assert p["n_host"] == want_round.count(HOST)
        assert p == model(hk, vl, 100)


def test_invalid_inputs():
    assert plan([0], [7], 1 << 20)[0] == EINVALID     # bytes without a kv
    assert plan([1], [7], 1 << 20, max_q=0)[0] == EINVALID


def test_random_against_model():
    rng = random.Random(21)
    for _ in range(300):
        n = rng.randrange(0, 60)
        arena = rng.randrange(1, 3000)
        max_q = rng.randrange(1, 25)
        hk = [rng.choice([0, 1, 1, 1]) for _ in range(n)]
        vl = [rng.choice([0, rng.randrange(0, 4000), rng.randrange(0, 200)]) if h
              else 0 for h in hk]
        want = model(hk, vl, arena, max_q)
        rc, got = plan(hk, vl, want["required"], arena, max_q)
        assert rc == OK and got == want
        rc, got = plan(hk, vl, want["required"] - 1, arena, max_q)
        assert rc == ENOBUF and got == want
        for lo, hi in want["rounds"]:
            assert 0 < sum(vl[lo:hi]) <= arena and lo // max_q == (hi - 1) // max_q
