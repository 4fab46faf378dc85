"""CPU test of the record hash of kb_digest_batch (include/kb_slab.h,
kdigest.h): the TEST-ONLY export kb_test_digest_record and
client.record_digest against a plain Python implementation of the spec, which
tests/test_gpu_digest_batch.py uses as its reference too. Needs no GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KLENS = [0, 1, 7, 8, 9, 95, 96, 97, 104, 300, 4096]
VLENS = [0, 1, 15, 16, 17, 255, 256, 257, 4095, 4097]

M = (1 << 64) - 1
G, SK, SV = 0x9E3779B97F4A7C15, 0x243F6A8885A308D3, 0x13198A2E03707344
S1, S2 = 0xA4093822299F31D0, 0x082EFA98EC4E6C89


def fmix(x):
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & M
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & M
    return x ^ (x >> 33)


def piece(b, S):
    return sum(fmix(int.from_bytes(b[8 * j:8 * j + 8], "little") ^ ((S + (j + 1) * G) & M))
               for j in range((len(b) + 7) // 8)) & M


def record(rev, key, val, keys_only=False):
    val = b"" if keys_only else val
    return fmix((fmix(rev ^ S1) + fmix(((len(key) << 32) | len(val)) ^ S2) +
                 piece(key, SK) + piece(val, SV)) & M)


def blob(tag, n):
    return bytes((tag * 7 + i * 13 + (i >> 8)) & 0xff for i in range(n))


@pytest.mark.parametrize("keys_only", [False, True])
@pytest.mark.parametrize("klen", KLENS)
def test_record_hash_matches_spec(klen, keys_only):
    import kubebrain_amd
    from kubebrain_amd import client
    f = C.CDLL(kubebrain_amd.build()).kb_test_digest_record
    f.restype = C.c_ulonglong
    for vlen in VLENS:
        # exact-size buffers: nothing readable lies behind the key or value
        key, val, rev = blob(klen, klen), blob(vlen + 1, vlen), 1000 + klen * vlen
        want = record(rev, key, val, keys_only)
        got = f(C.c_ulonglong(rev), key, C.c_size_t(klen), val, C.c_size_t(vlen),
                C.c_int(1 if keys_only else 0))
        assert got == want, (klen, vlen, keys_only)
        assert client.record_digest(rev, key, val, keys_only) == want
        assert (record(rev, key, val, True) == record(rev, key, val)) == (vlen == 0)


def test_kdigest_hostcheck(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    # the recipe of `make digest-hostcheck-asan`, built outside the tree
    src = os.path.join(REPO, "kubebrain_amd", "csrc", "kdigest_hostcheck.cc")
    exe = str(tmp_path / "kdigest_hostcheck")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                           "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "kdigest hostcheck OK" in out.stdout, out.stdout
