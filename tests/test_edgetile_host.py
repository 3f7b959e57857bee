"""The edge passes' tile decisions on the host (lsb_ostile.h).

tools/edgetile_host.cpp checks os_edge_applies, os_pass_tiles_ok and the rows
of either look-back track against brute force over small sorts: wherever the
rule admits a tile size, a run crosses at most one of the next pass's
sub-array boundaries.  A stand-alone host program, built with ASan/UBSan.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cxx in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++"), shutil.which("clang++")):
        if cxx and os.path.exists(cxx):
            return cxx
    raise AssertionError("no host C++ compiler")


def test_edge_tile_decisions_against_brute_force(tmp_path):
    exe = str(tmp_path / "edgetile_host")
    r = subprocess.run([_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "distributed-lsb_amd", "csrc"),
                        os.path.join(ROOT, "tools", "edgetile_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "edge tile host check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
