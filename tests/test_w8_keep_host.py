"""The rule by which the int8 W engine keeps what it made from S alone (csrc/eagle_host.h: w8_keep_valid, w8_declared_gen), on the host:
tests/host/test_w8_keep_host.cpp walks its truth table -- image, n, n_pad, workspace block and generation, S's content number, stream,
forget -- under ASan + UBSan, built as tests/test_bed_host.py builds its source."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "test_w8_keep_host.cpp")


def test_w8_keep_rule_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "w8_keep_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC,
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "w8 keep host checks passed" in r.stdout
