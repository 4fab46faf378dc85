"""CPU test of the arithmetic of kb_watch_batch (wreg.h): the global 64-event
chunk grid of k_wreg_scan re-aligned into each watcher's own 512-event refs.
wreg_hostcheck.cc proves it against the per-event construction kb_watch uses;
here it is built and run under the sanitizers. Needs no GPU."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wreg_hostcheck_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(REPO, "kubebrain_amd", "csrc", "wreg_hostcheck.cc")
    exe = str(tmp_path / "wreg_hostcheck")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
                           "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "wreg hostcheck OK" in out.stdout, out.stdout
