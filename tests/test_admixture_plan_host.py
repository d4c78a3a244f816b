"""The marker range plan of the admixture step's Q kernel, the part that needs no GPU.

tests/host/test_admix_host.cpp: csrc/eagle_host.h's admix_range_plan over n in {1, 16, 10000, ...} x L in {1, 15, 16, 17, 4097, 10^6, ...}
-- the ranges cover [0, L) exactly once, their boundaries are multiples of 16 and the partials buffer stays within admix_part_cap --
under ASan + UBSan, built as tests/test_windows_host.py builds its source: a stand-alone program, no preloaded runtime.
"""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "test_admix_host.cpp")


def test_admix_range_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "admix_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC,
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "admixture plan host checks passed" in r.stdout
