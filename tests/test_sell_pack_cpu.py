"""CPU: the packed entry stream's field arithmetic (csrc/kmcf_sell_pack.hpp: five 12-bit fields per 8-byte word),
checked by a stand-alone program (tests/sell_pack_check.cpp, its own main) built with the address and
undefined-behaviour sanitizers: rows of every length 0 ... 64, the extreme field values 0x000, 0xFFF, 0xBFF, 0x555 and
0xAAA in every field position, neighbouring fields and bits 60 ... 63 untouched, the step count ceil(len / 5)."""
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


def test_pack_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sell_pack_check")
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "sell_pack_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sell pack ok" in r.stdout
