"""The one owner of the library's device and pinned buffers (csrc/mfgp_own.h), on the host:
tests/own_main.cpp instantiates it over a counting fake instead of the HIP allocator, is
compiled here with the host compiler under AddressSanitizer and UBSan and run as a program
of its own. It checks that move construction and move assignment free exactly once, that
reset frees, release does not and swap frees nothing, that a self-move is harmless, that a
refused allocation leaves pointer null and size 0, and that the counts of what is held
return to zero; a double free or a leaked block ends it with the sanitizer's report.
CPU only: what the library itself holds on the device is counted by
tests/test_gpu_ownership.py."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_owner_frees_once_and_counts_return_to_zero(tmp_path):
    import __graft_entry__ as ge
    exe = tmp_path / "own_main"
    cxx = shutil.which("c++") or shutil.which("g++") or ge.HIPCC
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", ge.CSRC, os.path.join(HERE, "own_main.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
