"""CPU: the host decisions of the CG solver (csrc/kmcf_cgplan.hpp), checked by a stand-alone program
(tests/cgplan_check.cpp, its own main) built with the address and undefined-behaviour sanitizers: the path of a solve
(loop or resident launch, classic or single-reduction recurrence) for every kind of call over all combinations of its
boolean inputs, and how often the resident plan is asked on the way (the first question on a rank group is a
collective: 0 or 1 times, as DESIGN.md section 3.2 tabulates); kmcf_pcg_resident_applies' form of it; which solves leave
their last r.z to the caller's output kernel; the chunk schedule for limits 0 ... 100 under a stopping rule and for a
fixed iteration count; the peer-to-peer sequence numbers after a loop for the three protocols -- stop in the first
iteration, stop in the last one launched, end on the limit -- against numbers written out by hand, and that two solves
in a row keep them dense."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accelerated-kinetic-monte-carlo-simulations-of-atomistically-resolved-resistive-memory-arrays_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no C++ compiler for the stand-alone check")


def test_cgplan_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "cgplan_check")
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cgplan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cgplan ok" in r.stdout
