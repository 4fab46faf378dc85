"""The step's device chain: the wave-cooperative shadow
mark, the small-insert merge (k_delta_rank + k_delta_scatter) and the fused
gather of KB_GATHER_MODE=1. Every read is compared with the CPU oracle; the
fused gather's arena bytes also with the unchanged KB_GATHER_MODE=2 kernels.
The merge's slot arithmetic has a CPU check of its own (dmerge_hostcheck.cc,
run here as a stand-alone sanitizer build)."""
import os
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import benchwire as bw
import parity

parity.small_env()

gpu = pytest.mark.gpu
ROOT = b"/registry/pods/"


def val(tag, n):
    return bytes((tag * 13 + j * 7 + (j >> 8)) % 200 + 0x30 for j in range(n))


def key(ns, i):
    return ns + b"/obj-%05d" % i


def txn(d, rev, ops, chunk=400):
    """dual_txn in chunks; every op must succeed; rev[k] follows. A prev of
    None stands for the key's latest revision."""
    ops = [(k, rev[k] if p is None else p, v) for k, p, v in ops]
    for c0 in range(0, len(ops), chunk):
        part = ops[c0:c0 + chunk]
        out = bw.dual_txn(d, part)
        assert all(out), [o[0] for o, r in zip(part, out) if not r][:3]
        for (k, _p, _v), r in zip(part, out):
            rev[k] = r


def merge_now(d):
    """Any read uploads the staged rows: one delta merge."""
    d.count(ROOT + b"none/", ROOT + b"none0")


# ---- 1. shadow mark ----------------------------------------------------------
SM = ROOT + b"sm"
REVS = [1, 2, 63, 64, 65, 150]           # base revisions per key
SM_LONG = SM + b"/long-" + b"z" * 120    # > 96 B: tail in the spill heap
SM_P96 = (SM + b"/pair-").ljust(96, b"q")
SM_PAIR = [SM_P96 + b"a" * 10, SM_P96 + b"b" * 10]   # equal 96-byte prefixes
SM_LAST = ROOT + b"zzzz/last"           # the base run's last rows


@gpu
def test_shadow_mark_runs():
    d = bw.open_dual(KB_FLUSH_ROWS=1 << 16)
    try:
        rev = {}
        ks = {n: SM + b"/k-%03d" % n for n in REVS}
        other = [key(ROOT + b"sn", i) for i in range(40)]
        txn(d, rev, [(k, 0, val(i, i % 40)) for i, k in enumerate(other)])
        hist = {}
        for n, k in ks.items():          # n revisions each, one op per txn
            for g in range(n):
                txn(d, rev, [(k, rev.get(k, 0), val(n + g, (n + g) % 50))])
                hist.setdefault(k, []).append(rev[k])
        singles = [SM_LONG] + SM_PAIR
        txn(d, rev, [(k, 0, val(i, 20 + i)) for i, k in enumerate(singles)])
        for g in range(3):
            txn(d, rev, [(SM_LAST, rev.get(SM_LAST, 0), val(g, 9))])
        bw.flush(d.p)                    # everything sits in the base run
        p = bw.perf(d.p)
        assert p["delta_rows"] == 0 and p["base_rows"] > sum(REVS), p
        r_base = d.p.current_rev()
        # one more revision of each key, a key with no base row, the last key
        fresh = SM + b"/k-fresh"
        targets = list(ks.values()) + singles + [SM_LAST]
        ops = [(k, rev[k], val(77 + i, 30 + i)) for i, k in enumerate(targets)]
        ops.append((fresh, 0, val(5, 5)))
        txn(d, rev, ops)
        merge_now(d)                     # delta append + shadow mark
        p = bw.perf(d.p)
        assert p["delta_rows"] == 2 * len(ops), p
        qs = []
        for k in targets + [fresh]:
            old = hist[k][len(hist[k]) // 2] if k in hist else r_base
            for r in (0, rev[k], rev[k] - 1, old):
                d.list(k, k + b"0", r, 0)
                qs.append((k, k + b"0", r, 0))
        for ns in (SM, ROOT + b"zzzz", ROOT + b"sn"):
            for r in (0, r_base, r_base + 1, hist[ks[150]][70]):
                d.list(ns + b"/", ns + b"0", r, 0)
                qs.append((ns + b"/", ns + b"0", r, 0))
        # the same through the batched path: arena records against the oracle
        exp = bw.expected(d, qs, d.p.current_rev())
        bw.bench_range(d.p, qs, 0)
        bw.check_records(qs, exp, bw.last_range(d.p, 0))
        # a second update of a marked key keeps the smaller shadow revision
        r_first = rev[ks[150]]
        txn(d, rev, [(ks[150], rev[ks[150]], val(3, 3)), (SM_LAST, rev[SM_LAST], b"")])
        merge_now(d)
        for r in (0, r_first, r_first - 1):
            d.list(SM + b"/", SM + b"0", r, 0)
            d.list(ROOT + b"zzzz/", ROOT + b"zzzz0", r, 0)
        d.diff_dump()
    finally:
        d.close()


# ---- 2. small insert ---------------------------------------------------------
MID = ROOT + b"mid"
N_FILL = 1030                            # 2060 delta rows > 2048
MI_P96 = (ROOT + b"mil/pair-").ljust(96, b"w")
MI_PAIR = [MI_P96 + b"a" * 7, MI_P96 + b"b" * 300]
MI_NS = [ROOT + b"aaa", MID, ROOT + b"mil", ROOT + b"zzz"]


@gpu
@pytest.mark.parametrize("validate", [0, 1])
def test_small_insert(validate):
    d = bw.open_dual(KB_VALIDATE_DN=validate, KB_FLUSH_ROWS=1 << 16)
    try:
        rev = {}
        fill = [key(MID, 10 * i) for i in range(N_FILL)]
        z_last = key(ROOT + b"zzz", 99999)
        marks = []

        def grow():
            """The delta run back above 2048 rows (a dump folds it): every
            filler key and z_last get a new revision."""
            ops = [(k, rev.get(k, 0), val(i + len(marks), i % 24))
                   for i, k in enumerate(fill)]
            for c0 in range(0, N_FILL, 400):
                txn(d, rev, ops[c0:c0 + 400])
                merge_now(d)
            txn(d, rev, [(z_last, rev.get(z_last, 0), val(1, 8))])
            merge_now(d)
            p = bw.perf(d.p)
            assert p["delta_rows"] > 2048, p
            marks.append(d.p.current_rev())

        def check():
            cur = d.p.current_rev()
            for ns in MI_NS:
                for r in (0, marks[-1], marks[0], cur - 1):
                    d.list(ns + b"/", ns + b"0", r, 0)
                d.list(ns + b"/", ns + b"0", 0, 7)
                d.count(ns + b"/", ns + b"0")
            d.diff_dump()

        def batch(ops, small=1, big=0, rows=None):
            grow()
            p0 = bw.perf(d.p)
            txn(d, rev, ops, chunk=len(ops))
            merge_now(d)
            p1 = bw.perf(d.p)
            assert p1["folds"] == p0["folds"], (p0, p1)
            assert p1["merge_insert"] - p0["merge_insert"] == small, (p0, p1)
            assert p1["merge_big"] - p0["merge_big"] == big, (p0, p1)
            assert p1["merge_small"] == p0["merge_small"], (p0, p1)
            if not validate:
                assert p1["merges_async"] - p0["merges_async"] == 1, (p0, p1)
            if rows is not None:
                assert p1["delta_rows"] - p0["delta_rows"] == rows, (p0, p1)
            check()

        def fresh(ns, tag, n):
            return [(ns + b"/new-%s-%04d" % (tag, i), 0, val(i, i % 40))
                    for i in range(n)]

        # m = 2: one create (no replaced row), one update (rev-row replaced)
        batch(fresh(MID, b"one", 1), rows=2)
        batch([(fill[500], None, val(9, 9))], rows=1)
        # m = 1024: the largest small insert, spread over the whole run
        batch([(k + b"-x", 0, val(i, 16)) for i, k in enumerate(fill[:512])],
              rows=1024)
        # 513 ops = 1026 rows: the big path, untouched
        batch([(k + b"-y", 0, val(i, 16)) for i, k in enumerate(fill[:513])],
              small=0, big=1, rows=1026)
        # entirely in front of / behind every delta row
        batch(fresh(ROOT + b"aaa", b"front", 5), rows=10)
        batch([(z_last + b"-%d" % i, 0, val(i, 3)) for i in range(5)], rows=10)
        # rev-rows replaced: two adjacent delta keys and the owner of the
        # delta run's last row
        batch([(fill[10], None, val(1, 1)), (fill[11], None, val(2, 2)),
               (z_last, None, b"")], rows=3)
        # several new rows at one insertion point (between fill[20] and its
        # -x sibling), next to an update of fill[20] itself
        batch([(fill[20] + b"-a%d" % i, 0, val(i, 4)) for i in range(4)] +
              [(fill[20], None, val(3, 3))], rows=9)
        # long keys with equal 96-byte prefixes: create, then replace
        batch([(k, 0, val(i, 33)) for i, k in enumerate(MI_PAIR)], rows=4)
        grow()
        txn(d, rev, [(k, rev[k], val(i, 11)) for i, k in enumerate(MI_PAIR)])
        merge_now(d)                     # both pair keys now in the delta
        p0 = bw.perf(d.p)
        txn(d, rev, [(k, rev[k], val(i, 12)) for i, k in enumerate(MI_PAIR)])
        merge_now(d)
        p1 = bw.perf(d.p)
        assert p1["merge_insert"] - p0["merge_insert"] == 1, (p0, p1)
        assert p1["delta_rows"] - p0["delta_rows"] == 2, (p0, p1)
        check()
    finally:
        d.close()


# ---- 3. fused gather ---------------------------------------------------------
G0 = ROOT + b"g0"
G0_N = 2100
GV = ROOT + b"gv"
GL = ROOT + b"gl"
VLENS = [0, 1, 15, 16, 17, 100, 512, 1025]
GL_P96 = (GL + b"/pair-").ljust(96, b"p")
GL_KEYS = [GL + b"/long-" + b"x" * 100, GL_P96, GL_P96 + b"a", GL_P96 + b"b" * 204,
           GL + b"/short"]
CHUNK = 512                              # slab.hip GATHER_CH


def g_build(d):
    """Deterministic: every store built here holds the same rows at the same
    revisions. Base run + a delta of updates, creates and deletes."""
    rev = {}
    g0 = [key(G0, i) for i in range(G0_N)]
    gv = [key(GV, i) for i in range(64)]
    txn(d, rev, [(k, 0, val(i, i % 33)) for i, k in enumerate(g0)])
    txn(d, rev, [(k, 0, val(i, VLENS[i % 8])) for i, k in enumerate(gv)])
    txn(d, rev, [(k, 0, val(i, 40 + i)) for i, k in enumerate(GL_KEYS)])
    r_old = d.p.current_rev()
    bw.flush(d.p)
    txn(d, rev, [(k, rev[k], val(i + 1, (i + 5) % 33))
                 for i, k in enumerate(g0) if i % 7 == 3])
    txn(d, rev, [(k, rev[k], val(i + 2, VLENS[(i + 3) % 8]))
                 for i, k in enumerate(gv) if i % 3 == 1])
    txn(d, rev, [(GL_KEYS[0], rev[GL_KEYS[0]], val(8, 300)),
                 (GL_KEYS[2], rev[GL_KEYS[2]], b"")])
    merge_now(d)
    p = bw.perf(d.p)
    assert p["base_rows"] > 4000 and p["delta_rows"] > 600, p
    return {"rev": rev, "r_old": r_old, "cur": d.p.current_rev()}


def g_queries(info):
    r_old = info["r_old"]

    def rng(a, cnt, r=0, limit=0):
        if cnt == 0:                             # between two keys
            return (key(G0, a) + b"-", key(G0, a) + b"-z", r, limit)
        return (key(G0, a), key(G0, a + cnt), r, limit)

    qs = [rng(10 + 3 * i, c) for i, c in
          enumerate([0, 1, 255, 256, 257, 511, 512, 513])]
    qs += [(G0 + b"/", G0 + b"0", 0, 0),         # 2100 winners > 2 chunks
           rng(100, 1300, r_old, 0),             # three chunks, all base rows
           rng(0, 300, 0, 300),                  # exactly the limit
           rng(0, 400, 0, 300),                  # limit + 1: `more`
           rng(7, 2000, 0, 512),                 # 513 written: chunk + 1
           (GV + b"/", GV + b"0", 0, 0), (GV + b"/", GV + b"0", r_old, 0),
           (GL + b"/", GL + b"0", 0, 0), (GL_P96, GL_P96 + b"c", r_old, 2),
           (G0 + b"/zzz", G0 + b"/zzzz", 0, 0)]  # empty
    assert 2100 > 2 * CHUNK
    return qs


def run_and_check(d, qs, exp, mode, allow_overflow=()):
    bw.bench_range(d.p, qs, mode)
    raw = bw.last_range_raw(d.p, 0)
    got = bw.parse_wire(raw)
    bw.check_records(qs, exp, got, keys_only=bool(mode & 2),
                     allow_overflow=allow_overflow)
    if mode & 1:
        assert bw.last_range(d.p, 1) == got
    return raw, got


def written_bytes(raw):
    """The wire with every byte no gather kernel writes zeroed: a record's
    key and value are padded to 16 bytes, and the padding past the key's
    last 8-byte word and past the value is left as the arena held it."""
    out = bytearray(raw)
    (nq,) = struct.unpack_from("<I", raw, 0)
    off = 4 + nq * bw.HDR
    for q in range(nq):
        written, _total, nbytes, ovf, _z = struct.unpack_from("<qqqii", raw,
                                                              4 + q * bw.HDR)
        if ovf:
            continue
        end = off + nbytes
        for _ in range(written):
            _rev, klen, vlen = struct.unpack_from("<QII", raw, off)
            k0 = off + 16
            kw = k0 + (min(klen, 96) + 7) // 8 * 8 if klen <= 96 else k0 + klen
            v0 = k0 + bw.pad16(klen)
            out[kw:v0] = bytes(max(v0 - kw, 0))
            nxt = v0 + bw.pad16(vlen)
            out[v0 + vlen:nxt] = bytes(nxt - v0 - vlen)
            off = nxt
        assert off == end
    return bytes(out)


@pytest.fixture(scope="module")
def gworld():
    d = bw.open_dual(KB_FLUSH_ROWS=1 << 16)
    try:
        info = g_build(d)
        info["qs"] = g_queries(info)
        info["exp"] = bw.expected(d, info["qs"], info["cur"])
        info["raw"] = {}
        yield d, info
    finally:
        d.close()


@gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_fused_gather_records(gworld, mode):
    d, info = gworld
    qs, exp = info["qs"], info["exp"]
    want_n = [min(len(e), q[3] + 1) if q[3] else len(e) for q, e in zip(qs, exp)]
    assert want_n[:13] == [0, 1, 255, 256, 257, 511, 512, 513, 2100, 1300,
                           300, 301, 513], want_n
    raw, got = run_and_check(d, qs, exp, mode)
    info["raw"][mode] = raw
    vl = {len(v) for g in got for _r, _k, v in g[4]}
    if mode & 2:
        assert vl == {0}
    else:
        assert set(VLENS) <= vl, vl
    assert {len(k) for g in got for _r, k, _v in g[4]} >= {96, 97, 300}


KNOBS = {"t256": {"KB_GATHER_T": 256}, "t1024": {"KB_GATHER_T": 1024},
         "gw8": {"KB_GATHER_GW": 8}, "gw64": {"KB_GATHER_GW": 64}}


@gpu
@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_fused_gather_knobs(gworld, knob):
    _d, info = gworld
    d = bw.open_dual(KB_FLUSH_ROWS=1 << 16, **KNOBS[knob])
    try:
        mine = g_build(d)
        assert mine["cur"] == info["cur"]
        for mode in (0, 2):
            raw, _got = run_and_check(d, info["qs"], info["exp"], mode)
            if mode in info["raw"]:
                assert written_bytes(raw) == written_bytes(info["raw"][mode])
    finally:
        d.close()


@gpu
def test_fused_gather_equals_mode2(gworld):
    d1, info = gworld
    d = bw.open_dual(KB_FLUSH_ROWS=1 << 16, KB_GATHER_MODE=2)
    try:
        mine = g_build(d)
        assert mine["cur"] == info["cur"]
        for mode in (0, 2):
            raw2, _got = run_and_check(d, info["qs"], info["exp"], mode)
            raw1, _got = run_and_check(d1, info["qs"], info["exp"], mode)
            # directory, headers, keys, values, offsets: every written byte
            assert written_bytes(raw1) == written_bytes(raw2)
    finally:
        d.close()


@gpu
def test_fused_gather_overflow(gworld):
    _d, info = gworld
    arena = 1280 << 10
    d = bw.open_dual(KB_FLUSH_ROWS=1 << 16, KB_ARENA_BYTES=arena)
    try:
        mine = g_build(d)
        assert mine["cur"] == info["cur"]
        qs, exp = info["qs"], info["exp"]
        qcap = (arena // len(qs)) & ~15
        need = [sum(16 + bw.pad16(len(k)) + bw.pad16(len(v))
                    for _r, k, v in (e[:q[3] + 1] if q[3] else e))
                for q, e in zip(qs, exp)]
        over = {i for i, n in enumerate(need) if n > qcap}
        # single-chunk and multi-chunk queries on both sides of the share
        assert over == {8, 9}, (qcap, need)
        _raw, got = run_and_check(d, qs, exp, 0, allow_overflow=over)
        for i in over:                   # the byte count is still reported
            assert got[i][2] == need[i] and got[i][3], (i, got[i][:4])
        # keys-only records are smaller: fewer queries overflow
        need_k = [sum(16 + bw.pad16(len(k))
                      for _r, k, _v in (e[:q[3] + 1] if q[3] else e))
                  for q, e in zip(qs, exp)]
        over_k = {i for i, n in enumerate(need_k) if n > qcap}
        assert over_k == {8}, (qcap, need_k)
        run_and_check(d, qs, exp, 2, allow_overflow=over_k)
    finally:
        d.close()


# ---- 4. the slot arithmetic on the CPU ----------------------------------------
def test_dmerge_hostcheck_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "kubebrain_amd", "csrc", "dmerge_hostcheck.cc")
    exe = str(tmp_path / "dmerge_hostcheck")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                           "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "dmerge hostcheck OK" in out.stdout, out.stdout
