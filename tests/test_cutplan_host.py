"""k_onesweep's cut plans on the host (lsb_ostile.h).

A bucket thread works out where its runs of one sub-array meet the next
pass's sub-array boundaries once, when its workgroup enters the sub-array
(os_cut_plan), and then cuts each tile's run by two compares (os_cut) instead
of calling os_run_cut per tile.  tools/cutplan_host.cpp compares both forms of
os_cut with os_run_cut word for word: next-pass tiles of 4096, 4608 and 5120
records, 1 to 40 tiles whole and ragged, 61,441 and 300,007 records, every
range and run on a grid at -1, 0 and +1 around each of the seven boundaries,
counts up to the tile size, and ranges over two boundaries, which must report
`general`.  A stand-alone host program, built with ASan/UBSan.
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


def test_cut_plans_against_os_run_cut(tmp_path):
    exe = str(tmp_path / "cutplan_host")
    r = subprocess.run([_compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "distributed-lsb_amd", "csrc"),
                        os.path.join(ROOT, "tools", "cutplan_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cut plan host check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
