"""The row windows of a pass over an ingested image, the part that needs no GPU.

tests/host/test_windows_host.cpp: csrc/eagle_host.h's RowWindows (disjoint, overlapped and core / halo windows) against window lists
written out by hand and against the three loops the entry points used to carry, under ASan + UBSan, built as tests/test_bed_host.py
builds its source.
"""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "test_windows_host.cpp")


def test_row_windows_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "windows_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC,
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "window host checks passed" in r.stdout
