"""CPU check of tests/benchwire.py: the parser of the kb_test_last_range wire
round-trips a hand-built buffer and rejects damaged ones (no GPU)."""
import struct

import pytest

import benchwire as bw

K97 = b"/registry/pods/ns-00/" + b"k" * (97 - 21)
QUERIES = [
    # (written, total, overflow, records)
    (3, 3, False, [(1001, b"/registry/a", b"v" * 17),
                   (1002, K97, b""),                    # 97-byte key, empty value
                   (1003, b"/registry/c" + b"c" * 5, b"x" * 16)]),
    (0, 0, False, []),
    (40, 40, True, [(7, b"/registry/big", b"z" * 4097)]),  # overflowed: no bytes
    (1, 9, False, [(2 ** 40 + 5, b"/registry/d", b"\x00\xff" * 50)]),
]


def test_roundtrip():
    assert len(K97) == 97
    raw = bw.build_wire(QUERIES)
    got = bw.parse_wire(raw)
    assert len(got) == 4
    for (w, t, ovf, recs), (gw, gt, gb, govf, grecs) in zip(QUERIES, got):
        assert (gw, gt, govf) == (w, t, ovf)
        if ovf:
            assert grecs == [] and gb > 0
        else:
            assert grecs == recs
            assert gb == sum(16 + bw.pad16(len(k)) + bw.pad16(len(v))
                             for _, k, v in recs)
    # the 97-byte key takes 112 key bytes, the empty value none
    assert got[0][2] == (16 + 16 + 32) + (16 + 112 + 0) + (16 + 16 + 16)
    # padding is never part of a key or value
    assert all(b"\xa5" not in k + v for _, _, _, _, r in got for _, k, v in r)


def test_empty_batch():
    assert bw.parse_wire(struct.pack("<I", 0)) == []


@pytest.mark.parametrize("cut", [1, 15, 16, 17, 64, 200])
def test_truncated_raises(cut):
    raw = bw.build_wire(QUERIES)
    with pytest.raises(ValueError):
        bw.parse_wire(raw[:-cut])


def test_truncated_directory_raises():
    raw = bw.build_wire(QUERIES)
    for n in (0, 3, 4, 4 + 31, 4 + 4 * 32 - 1):
        with pytest.raises(ValueError):
            bw.parse_wire(raw[:n])


def test_inconsistent_raises():
    raw = bytearray(bw.build_wire(QUERIES))
    with pytest.raises(ValueError):           # trailing bytes
        bw.parse_wire(bytes(raw) + b"\0" * 16)
    bad = bytearray(raw)
    struct.pack_into("<q", bad, 4 + 16, 16)   # query 0 claims fewer bytes
    with pytest.raises(ValueError):
        bw.parse_wire(bytes(bad))
    bad = bytearray(raw)
    struct.pack_into("<q", bad, 4, 2)         # query 0 claims fewer records
    with pytest.raises(ValueError):
        bw.parse_wire(bytes(bad))
    bad = bytearray(raw)
    struct.pack_into("<I", bad, 4 + 4 * 32 + 8, 5000)  # first klen runs away
    with pytest.raises(ValueError):
        bw.parse_wire(bytes(bad))


def test_pack_layouts():
    q = bw.pack_queries([(b"ab", b"abc", 7, 500)])
    assert q == struct.pack("<IIQQ", 2, 3, 7, 500) + b"ab" + b"abc"
    t = bw.pack_txns([(b"key", 9, b"va")])
    assert t == struct.pack("<IQI", 3, 9, 2) + b"key" + b"va"
    assert bw.pack_dels([(b"key", 9)]) == struct.pack("<IQ", 3, 9) + b"key"
