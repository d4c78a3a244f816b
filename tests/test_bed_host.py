"""PLINK binary (.bed/.bim/.fam) ingestion, the part that needs no GPU.

  * tests/host/test_bed_host.cpp: the HIP-free pieces of eagle_create_ascii_from_bed (csrc/eagle_host.h: header check, expected
    size, row strides, window arithmetic) under ASan + UBSan, built as tests/test_host_sanitizers.py builds its source;
  * r_api.ReadBim, the .fam/.bim counting and the "could not be found" exits of ReadMarker(type="PLINKbed") on the committed
    fixture tests/golden/plink_150x100.* (written by tests/golden/make_plink_bed.py from geno_150x100.txt);
  * synth.write_bed against the numpy decoder of tests/test_gpu_bed.py.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_gpu_bed import decode_bed
from conftest import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tests", "host", "test_bed_host.cpp")
PREFIX = os.path.join(GOLDEN, "plink_150x100")


def test_bed_host_pieces_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "bed_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC,
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bed host checks passed" in r.stdout


def test_fixture_is_the_text_panel():
    """The committed .bed holds geno_150x100.txt: digit 0 -> 00, 1 -> 10, 2 -> 11, nothing missing, pad fields zero."""
    digits, missing = decode_bed(PREFIX + ".bed", 150, 100)
    table = np.loadtxt(os.path.join(GOLDEN, "geno_150x100.txt"), dtype=np.uint8)
    assert np.array_equal(digits.T, table) and not missing.any()
    raw = np.fromfile(PREFIX + ".bed", dtype=np.uint8)[3:].reshape(100, 38)
    assert not (raw[:, 37] >> 4).any()   # n = 150: two pad fields in every row's last byte


def test_read_bim_and_counts():
    from eagleeverything_amd import r_api
    m = r_api.ReadBim(PREFIX + ".bim")
    assert sorted(m) == ["Chr", "Pos", "SNP"] and all(len(v) == 100 for v in m.values())
    assert m["SNP"][0] == "rs1001" and m["SNP"][99] == "rs1100" and m["Chr"][24:26] == ["1", "2"] and m["Pos"][2] == 30000
    assert r_api._count_lines(PREFIX + ".fam") == 150 and r_api._count_lines(PREFIX + ".bim") == 100
    assert r_api.bed_fileset(PREFIX) == r_api.bed_fileset(PREFIX + ".bed") == (PREFIX + ".bed", PREFIX + ".bim", PREFIX + ".fam")


def test_count_lines_follows_getline(tmp_path):
    from eagleeverything_amd import r_api
    p = tmp_path / "x.fam"
    for text, lines in (("", 0), ("a b\n", 1), ("a b\nc d", 2), ("a\n\nb\n", 3)):
        p.write_text(text)
        assert r_api._count_lines(str(p)) == lines


def test_read_bim_rejects_short_lines(tmp_path):
    from eagleeverything_amd import r_api
    p = tmp_path / "x.bim"
    p.write_text("1 rs1 0 100 A B\n1 rs2 0\n")
    with pytest.raises(ValueError, match="line 2"):
        r_api.ReadBim(str(p))


@pytest.mark.parametrize("gone", [".bim", ".fam", ".bed"])
def test_readmarker_bed_missing_companion(tmp_path, gone):
    """A missing file of the set ends like the other "could not be found" exits: the message, then None -- before any device work."""
    from eagleeverything_amd import r_api
    for ext in (".bed", ".bim", ".fam"):
        if ext != gone:
            shutil.copy(PREFIX + ext, str(tmp_path / ("p" + ext)))
    for name in ("p.bed", "p"):
        msgs = []
        assert r_api.ReadMarker(str(tmp_path / name), type="PLINKbed", message=msgs.append) is None
        assert any("p%s could not be found" % gone in m for m in msgs) and "terminated with errors" in msgs[-1]
    assert not (tmp_path / "M.ascii").exists()


def test_readmarker_unknown_type_message_is_unchanged():
    from eagleeverything_amd import r_api
    msgs = []
    assert r_api.ReadMarker(PREFIX + ".bed", type="bed", message=msgs.append) is None
    assert msgs == [' type must be set to "text" or "PLINK". \n', " ReadMarker has terminated with errors"]


@pytest.mark.parametrize("n", [8, 9, 10, 11, 150])
def test_write_bed_round_trip(tmp_path, n):
    from eagleeverything_amd import r_api, synth
    L = 37
    Mt8 = synth.genotypes_marker_major(n, L, seed=n)
    rng = np.random.default_rng(n)
    miss = rng.random((L, n)) < 0.1
    for tag, mask in (("full", None), ("miss", miss)):
        bed = synth.write_bed(str(tmp_path / tag), Mt8, missing=mask)
        assert os.path.getsize(bed) == 3 + L * ((n + 3) // 4)
        digits, missing = decode_bed(bed, n, L)
        want = (Mt8 + 1).astype(np.uint8)
        if mask is not None:
            want[mask] = 1
        assert np.array_equal(digits, want)
        assert np.array_equal(missing, mask if mask is not None else np.zeros((L, n), dtype=bool))
        raw = np.fromfile(bed, dtype=np.uint8)[3:].reshape(L, -1)
        if n % 4:
            assert not (raw[:, -1] >> (2 * (n % 4))).any()   # pad fields are zero
        assert r_api._count_lines(str(tmp_path / tag) + ".fam") == n
        assert len(r_api.ReadBim(str(tmp_path / tag) + ".bim")["SNP"]) == L
