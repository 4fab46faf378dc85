"""CPU test of the tile map of kb_count_batch (cplan.h), through the TEST-ONLY
export kb_test_count_plan, against a Python model: a launch of nq queries has
2 nq row segments (per query the base run's [lo, hi) then the delta run's
[dlo, dhi)), every segment is cut into tiles of T rows, and an exclusive prefix
over the segments' tile counts numbers the tiles. Needs no GPU."""
import ctypes as C
import os
import random
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OK, EINVALID, ENOBUF = 0, 5, 100
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import kubebrain_amd
    return C.CDLL(kubebrain_amd.build())


def plan(bounds, T, tile_cap=None):
    """bounds = [(lo, hi, dlo, dhi)] -> (rc, pfx, [(query, run, r0, r1)])."""
    lib = _lib()
    nq = len(bounds)
    flat = [v for b in bounds for v in b]
    arr = (C.c_longlong * max(len(flat), 1))(*flat)
    pfx = (C.c_ulonglong * (2 * nq + 1))(*([12345] * (2 * nq + 1)))
    want = model(bounds, T)[1] if tile_cap is None else None
    cap = len(want) if tile_cap is None else tile_cap
    m = max(cap, 1)
    tq, tr = (C.c_int * m)(*([-7] * m)), (C.c_int * m)(*([-7] * m))
    r0, r1 = (C.c_longlong * m)(*([-7] * m)), (C.c_longlong * m)(*([-7] * m))
    nt = C.c_size_t(12345)
    f = lib.kb_test_count_plan
    f.restype = C.c_int
    rc = f(arr, C.c_size_t(nq), C.c_longlong(T), pfx, tq, tr, r0, r1,
           C.c_size_t(cap), C.byref(nt))
    if rc == EINVALID:
        return rc, None, None
    tiles = [(tq[i], tr[i], r0[i], r1[i]) for i in range(min(nt.value, cap))]
    if rc == ENOBUF:
        assert nt.value > cap
        assert all(t == (-7, -7, -7, -7) for t in tiles)   # nothing written
        return rc, list(pfx), nt.value
    assert nt.value == len(tiles)
    return rc, list(pfx), tiles


def model(bounds, T):
    """Independent model: walk the segments, cut each into T-row tiles."""
    pfx, tiles = [0], []
    for q, (lo, hi, dlo, dhi) in enumerate(bounds):
        for run, (a, b) in enumerate(((lo, hi), (dlo, dhi))):
            r = a
            while r < b:
                tiles.append((q, run, r, min(r + T, b)))
                r += T
            pfx.append(len(tiles))
    return pfx, tiles


def check(bounds, T):
    rc, pfx, tiles = plan(bounds, T)
    assert rc == OK
    want_pfx, want_tiles = model(bounds, T)
    assert pfx == want_pfx
    assert tiles == want_tiles
    # the issue's formula for a segment's tile count, inverted bounds included
    segs = [s for b in bounds for s in ((b[0], b[1]), (b[2], b[3]))]
    for s, (a, b) in enumerate(segs):
        assert pfx[s + 1] - pfx[s] == max(0, b - a + T - 1) // T
    rows = sum(max(0, b - a) for a, b in segs)
    assert sum(r1 - r0 for _, _, r0, r1 in tiles) == rows
    assert all(r0 < r1 for _, _, r0, r1 in tiles)
    assert -(-rows // T) <= len(tiles) <= rows // T + len(segs)
    return pfx, tiles


@pytest.mark.parametrize("T", [64, 128, 4096])
def test_segment_lengths_around_the_tile(T):
    lens = [0, 1, T - 1, T, T + 1, 3 * T, 3 * T + 1]
    for la in lens:
        for lb in lens:
            for off in (0, 1, 63, 1 << 33):
                check([(off, off + la, 5, 5 + lb)], T)
                check([(off, off + la, 5, 5 + lb), (9, 9 + lb, off, off + la)], T)


@pytest.mark.parametrize("T", [64, 128, 4096])
def test_inverted_and_empty_bounds(T):
    pfx, tiles = check([(10, 3, 0, 0)], T)
    assert pfx == [0, 0, 0] and tiles == []
    check([(T + 1, 0, 7, 7)], T)
    check([(T + 5, T + 4, 100, 100 + T)], T)            # lo = hi + 1: no tile
    pfx, tiles = check([(5, 5 + T, 9, 2), (1, 0, 3, 3 + 2 * T + 1)], T)
    assert pfx == [0, 1, 1, 1, 4]
    assert tiles[0] == (0, 0, 5, 5 + T) and tiles[-1] == (1, 1, 3 + 2 * T, 3 + 2 * T + 1)
    pfx, tiles = check([], T)
    assert pfx == [0] and tiles == []


def test_1024_queries():
    rng = random.Random(5)
    for T in (64, 128, 4096):
        bounds = []
        for q in range(1024):
            lo, dlo = rng.randrange(0, 100000), rng.randrange(0, 3000)
            ln = rng.choice([0, 1, T - 1, T, T + 1, rng.randrange(0, 5 * T)])
            dl = rng.choice([0, 0, 1, T, rng.randrange(0, 2 * T)])
            if q % 17 == 3:
                bounds.append((lo + ln, lo, dlo + dl, dlo))   # inverted
            else:
                bounds.append((lo, lo + ln, dlo, dlo + dl))
        pfx, tiles = check(bounds, T)
        assert len(pfx) == 2049
        assert len(tiles) > 1024


def test_random_against_model():
    rng = random.Random(11)
    for _ in range(200):
        T = 64 * rng.randrange(1, 9)
        nq = rng.choice([1, 2, 3, 9])
        bounds = [tuple(rng.randrange(0, 1500) for _ in range(4)) for _ in range(nq)]
        check(bounds, T)


def test_invalid_tile_and_enobuf():
    for T in (0, 1, 63, 65, 100, -64):
        assert plan([(0, 10, 0, 0)], T, tile_cap=8)[0] == EINVALID, T
    rc, pfx, n_tiles = plan([(0, 300, 0, 70)], 64, tile_cap=6)
    assert rc == ENOBUF and n_tiles == 7 and pfx == [0, 5, 7]
    rc, pfx, tiles = plan([(0, 300, 0, 70)], 64, tile_cap=7)
    assert rc == OK and len(tiles) == 7


def test_cplan_hostcheck_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(REPO, "kubebrain_amd", "csrc", "cplan_hostcheck.cc")
    exe = str(tmp_path / "cplan_hostcheck")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                           "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "cplan hostcheck OK" in out.stdout, out.stdout
