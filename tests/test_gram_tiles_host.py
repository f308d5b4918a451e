"""CPU: the Gram tile order of csrc/grf_gram_tiles.h, host side only.

tests/gram_tiles_host_main.cpp is built with the host compiler alone (the header is plain C++) and run once.  It
enumerates every tile of every launch shape below band by band and asks both locate forms -- the generic 64-bit
one and the 32-bit one from host constants, the latter also with its square-root estimate moved 0.4 either way,
which covers a device square root that is a few ulp off -- for the same (band, row):

* rows in {1, 63, 64, 65, 129, 4095, 4096, 4097, 8193, 12289}, W in {64, 128, 4096}, symmetric and full mode,
  the square case and two bands more, J_off in {0, 2}, each launch cut into 1, 3 and 7 parts;
* n = 10^6 and 3 * 10^6 at W = 4096: the tiles within 2 of every band boundary and 10^4 seeded random tiles;
* n = 5 * 10^6 at W = 4096 (3.05e9 tiles): the whole launch must take the 64-bit form, a part ending below 2^31
  the 32-bit form, a part across 2^31 the 64-bit form.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "efficient-gaussian-process-on-graphs_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "gram_tiles_host_main.cpp")


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler (c++, g++ or clang++) on PATH")


def test_both_locate_forms_agree_with_the_enumeration(tmp_path):
    exe = str(tmp_path / "gram_tiles_host")
    subprocess.run([_host_compiler(), "-O2", "-std=c++17", "-Wall", "-I", CSRC, MAIN, "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok" and lines[0].startswith("enumerated ")
    assert int(lines[0].split()[1]) > 10 ** 8  # (nothing left out: 119 M tiles over the listed shapes)
