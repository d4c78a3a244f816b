"""PLINK binary ingestion on the GPU: eagle_create_ascii_from_bed / ReadMarker(type="PLINKbed") (k_bed_decode on the hot path).

Expected values come from two places that do not share code with the feature: the numpy decoder below (the bed format restated
in twenty lines) and the library's own text route, which the reference pins (tests/test_ingest.py).
"""
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN

PREFIX = os.path.join(GOLDEN, "plink_150x100")
TXT = os.path.join(GOLDEN, "geno_150x100.txt")
E2B_HEADER = 64


# ---- the decoder: .bed, SNP-major = bytes 0x6c 0x1b 0x01, then ceil(n/4) bytes per marker; individual 4b+q sits at bits 2q of
# byte b of its marker's row; code 00 = homozygous A1, 01 = missing, 10 = heterozygous, 11 = homozygous A2 ----
def decode_bed(path, n, L):
    """-> (digits, missing): L x n uint8 genotype digits 0/1/2 with missing as 1 (the reference's missing -> heterozygote rule),
    and the L x n boolean mask of the missing ones."""
    raw = np.fromfile(path, dtype=np.uint8)
    rb = (n + 3) // 4
    assert raw.size == 3 + L * rb and tuple(raw[:3]) == (0x6c, 0x1b, 0x01)
    rows = raw[3:].reshape(L, rb)
    codes = np.stack([(rows >> (2 * q)) & 3 for q in range(4)], axis=2).reshape(L, 4 * rb)[:, :n]
    digits = np.array([0, 1, 1, 2], dtype=np.uint8)[codes]
    return digits, codes == 1


def text_bytes(digits):
    """The bytes of a genotype text file whose lines are the rows of `digits`."""
    rows, cols = digits.shape
    buf = np.empty((rows, cols + 1), dtype=np.uint8)
    buf[:, :cols] = digits + ord("0")
    buf[:, cols] = ord("\n")
    return buf.tobytes()


def sidecar_payload(digits):
    """The rows of the 2-bit sidecar of that text file: code = digit, column 4b+q at bits 2q of byte b, rows padded to 16 bytes."""
    rows, cols = digits.shape
    rb16 = ((cols + 3) // 4 + 15) // 16 * 16
    f = np.zeros((rows, 4 * rb16), dtype=np.uint8)
    f[:, :cols] = digits
    f = f.reshape(rows, rb16, 4)
    return (f[:, :, 0] | f[:, :, 1] << 2 | f[:, :, 2] << 4 | f[:, :, 3] << 6).astype(np.uint8).tobytes()


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _panel(tmp_path, n, L, p_missing, seed):
    from eagleeverything_amd import synth
    Mt8 = synth.genotypes_marker_major(n, L, seed=seed)
    miss = np.random.default_rng(seed).random((L, n)) < p_missing if p_missing else None
    return synth.write_bed(str(tmp_path / "panel"), Mt8, missing=miss)


WARNING = " Warning:  PLINK file contains missing alleles (i.e. 0 or - ) "


# ------------------------------------------------------------------------------------------------ 4. the committed fixture
@pytest.mark.gpu
def test_gpu_bed_fixture_equals_text_route(golden, tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    g = golden("geno_150x100")
    d_bed, d_txt = tmp_path / "bed", tmp_path / "txt"
    d_bed.mkdir(), d_txt.mkdir()
    msgs = []
    geno = r_api.ReadMarker(PREFIX + ".bed", type="PLINKbed", outdir=str(d_bed), message=msgs.append, quiet=False)
    assert geno is not None and geno["dim_of_ascii_M"] == [150, 100]
    assert any("Summary of Marker File" in m for m in msgs) and any("The marker file has been Uploaded" in m for m in msgs)
    assert WARNING not in msgs
    # right after ingestion: MM^T (trace 9748, maximum 89) and the scan, before the text route touches the device
    MMt = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 4, np.nan, (150, 100))
    assert np.trace(MMt) == 9748 and MMt.max() == 89 and np.array_equal(MMt, g["MMt"].astype(np.float64))
    out = rcpp_api.calculate_a_and_vara_rcpp(geno["asciifileMt"], np.nan, g["S"], g["V"], 8.0, (100, 150), g["ahat"])
    rcpp_api.drop_cache()
    ref_geno = r_api.ReadMarker(TXT, type="text", AA=0, AB=1, BB=2, outdir=str(d_txt))
    ref = rcpp_api.calculate_a_and_vara_rcpp(ref_geno["asciifileMt"], np.nan, g["S"], g["V"], 8.0, (100, 150), g["ahat"])
    assert np.array_equal(out["a"], ref["a"]) and np.array_equal(out["vara"], ref["vara"])   # bit for bit
    for key in ("asciifileM", "asciifileMt"):
        assert _read(geno[key]) == _read(ref_geno[key])
        a, b = _read(geno[key] + ".e2b"), _read(ref_geno[key] + ".e2b")
        assert len(a) == len(b) and a[E2B_HEADER:] == b[E2B_HEADER:]
        assert a[:48] == b[:48]   # magic, version, rows, cols, row_bytes, src_size; src_mtime_ns (the text file's stamp) follows
    # the prefix names the same fileset
    geno2 = r_api.ReadMarker(PREFIX, type="PLINKbed", outdir=str(d_bed))
    assert geno2 == geno
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 5. random panels
@pytest.mark.gpu
@pytest.mark.parametrize("n,L", [(37, 53), (301, 1999), (1030, 777), (2049, 5000)])
def test_gpu_bed_random_panels(tmp_path, n, L):
    from eagleeverything_amd import rcpp_api
    bed = _panel(tmp_path, n, L, 0.03, seed=n * 1000 + L)
    digits, missing = decode_bed(bed, n, L)
    fM, fMt = str(tmp_path / "M.ascii"), str(tmp_path / "Mt.ascii")
    msgs = []
    n_missing = rcpp_api.create_ascii_from_bed(bed, fM, fMt, 8.0, [n, L], message=msgs.append)
    assert n_missing == int(missing.sum()) and n_missing > 0
    assert msgs.count(WARNING) == 1
    assert any("As an approximation, AMpus has set these missing genotypes to heterozygotes." in m for m in msgs)
    assert _read(fMt) == text_bytes(digits)
    assert _read(fM) == text_bytes(np.ascontiguousarray(digits.T))
    assert _read(fMt + ".e2b")[E2B_HEADER:] == sidecar_payload(digits)
    assert _read(fM + ".e2b")[E2B_HEADER:] == sidecar_payload(np.ascontiguousarray(digits.T))
    # the adopted images are what the files hold
    MMt = rcpp_api.calculateMMt_rcpp(fM, 8.0, 4, np.nan, (n, L))
    M = digits.T.astype(np.int64) - 1
    assert np.array_equal(MMt, (M @ M.T).astype(np.float64))
    blk = rcpp_api.ReadBlock(fMt, 3, n, min(40, L - 3))
    assert np.array_equal(blk, M.T[3:3 + min(40, L - 3)].astype(np.float64))
    rcpp_api.drop_cache()


@pytest.mark.gpu
def test_gpu_bed_without_missing_sends_no_warning(tmp_path):
    from eagleeverything_amd import rcpp_api
    n, L = 301, 1999
    bed = _panel(tmp_path, n, L, 0.0, seed=11)
    digits, missing = decode_bed(bed, n, L)
    assert not missing.any()
    msgs = []
    assert rcpp_api.create_ascii_from_bed(bed, str(tmp_path / "M.ascii"), str(tmp_path / "Mt.ascii"), 8.0, [n, L], message=msgs.append) == 0
    assert not any("missing alleles" in m or "missing genotypes" in m for m in msgs)   # (the directory's own name says "missing")
    assert _read(tmp_path / "Mt.ascii") == text_bytes(digits) and _read(tmp_path / "M.ascii") == text_bytes(np.ascontiguousarray(digits.T))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 6. the non-resident M path
@pytest.mark.gpu
def test_gpu_bed_bands_and_windows_equal_resident_run(tmp_path, monkeypatch):
    """EAGLE_HIP_MAX_RESIDENT_GB = 0.0005 (500,000 bytes) at n = 1030 (n_pad 1280), L = 2100 (L_pad 2304): marker windows of
    max(256, 500,000 / 1280 rounded down to 256) = 256, which does not divide 2,100 (nine windows, the last of 52 markers), and an
    image of M of 256 individuals per pass over the bed file (five passes), neither image kept."""
    from eagleeverything_amd import rcpp_api
    n, L = 1030, 2100
    bed = _panel(tmp_path, n, L, 0.03, seed=6)
    digits, missing = decode_bed(bed, n, L)
    d_res, d_band = tmp_path / "resident", tmp_path / "bands"
    d_res.mkdir(), d_band.mkdir()
    rcpp_api.drop_cache()
    m_res = rcpp_api.create_ascii_from_bed(bed, str(d_res / "M.ascii"), str(d_res / "Mt.ascii"), 8.0, [n, L])
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.0005")
    msgs = []
    m_band = rcpp_api.create_ascii_from_bed(bed, str(d_band / "M.ascii"), str(d_band / "Mt.ascii"), 8.0, [n, L], message=msgs.append)
    assert m_res == m_band == int(missing.sum()) and msgs.count(WARNING) == 1
    for name in ("M.ascii", "Mt.ascii"):
        assert _read(d_res / name) == _read(d_band / name)
        a, b = _read(str(d_res / name) + ".e2b"), _read(str(d_band / name) + ".e2b")
        assert a[E2B_HEADER:] == b[E2B_HEADER:] and a[:48] == b[:48]
    assert _read(d_band / "Mt.ascii") == text_bytes(digits) and _read(d_band / "M.ascii") == text_bytes(np.ascontiguousarray(digits.T))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 7. error exits (all decided on the host)
@pytest.mark.gpu
def test_gpu_bed_error_exits(tmp_path):
    from eagleeverything_amd import rcpp_api
    ERR_OPEN, ERR_FORMAT, ERR_ARG = -1, -2, -3
    good = _read(PREFIX + ".bed")
    fM, fMt = str(tmp_path / "M.ascii"), str(tmp_path / "Mt.ascii")

    def attempt(name, data, dims, code, *words):
        p = tmp_path / name
        if data is not None:
            p.write_bytes(data)
        with pytest.raises(rcpp_api.EagleError) as e:
            rcpp_api.create_ascii_from_bed(str(p), fM, fMt, 8.0, dims)
        assert e.value.code == code, e.value
        assert "\n" not in e.value.text.strip() and all(w in e.value.text for w in words), e.value.text
        assert not os.path.exists(fM + ".e2b") and not os.path.exists(fMt + ".e2b")
        for f in (fM, fMt):
            assert not os.path.exists(f) or os.path.getsize(f) == 0

    attempt("absent.bed", None, [150, 100], ERR_OPEN, "absent.bed")
    attempt("magic.bed", b"\x6c\x1c\x01" + good[3:], [150, 100], ERR_FORMAT, "0x6c 0x1b")
    attempt("text.bed", _read(TXT), [150, 100], ERR_FORMAT, "0x6c 0x1b")
    attempt("indmajor.bed", b"\x6c\x1b\x00" + good[3:], [150, 100], ERR_FORMAT, "individual-major")
    attempt("short.bed", good[:-1], [150, 100], ERR_FORMAT, "3802", "3803")
    attempt("long.bed", good + b"\x00", [150, 100], ERR_FORMAT, "3804", "3803")
    attempt("dims.bed", good, [150, 99], ERR_FORMAT, "3803", "3765")
    attempt("dims.bed", good, [153, 100], ERR_FORMAT, "3803", "3903")
    attempt("empty.bed", b"", [150, 100], ERR_FORMAT)
    attempt("two.bed", b"\x6c\x1b", [150, 100], ERR_FORMAT)
    attempt("good.bed", good, [0, 100], ERR_ARG)
    attempt("good.bed", good, [150, 0], ERR_ARG)
    attempt("good.bed", good, [-1, 100], ERR_ARG)
    # a failed call after a good one leaves no sidecar of the good one behind a text file it cut back
    assert rcpp_api.create_ascii_from_bed(str(tmp_path / "good.bed"), fM, fMt, 8.0, [150, 100]) == 0
    assert os.path.exists(fM + ".e2b") and os.path.getsize(fM) == 150 * 101
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 8. end to end
@pytest.mark.gpu
def test_gpu_bed_to_am_and_summary(tmp_path):
    """AM() on the fixture ingested from bed picks what it picks on the same panel ingested from text (a trait planted as
    tests/test_am_driver.py plants its own), and SummaryAM(map=ReadBim(...)) names the picks as the .bim does."""
    from eagleeverything_amd import am, r_api, rcpp_api
    d_bed, d_txt = tmp_path / "bed", tmp_path / "txt"
    d_bed.mkdir(), d_txt.mkdir()
    M8 = np.loadtxt(TXT, dtype=np.int8) - 1
    n = M8.shape[0]
    qtl = [20, 70]
    y = 1.5 * M8[:, qtl[0]] - 1.2 * M8[:, qtl[1]] + 0.5 * np.random.default_rng(4).standard_normal(n)
    X = np.ones((n, 1))
    geno_txt = r_api.ReadMarker(TXT, type="text", AA=0, AB=1, BB=2, outdir=str(d_txt))
    ref = am.AM(y, X, geno_txt, maxit=6)
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(PREFIX, type="PLINKbed", outdir=str(d_bed))
    res = am.AM(y, X, geno, maxit=6)
    assert res["all_picks"] == ref["all_picks"] and res["selected_loci"] == ref["selected_loci"]
    assert res["extBIC_trace"] == ref["extBIC_trace"]
    assert set(q + 1 for q in qtl) <= set(res["selected_loci"])
    bim = r_api.ReadBim(PREFIX + ".bim")
    msgs = []
    got = r_api.SummaryAM(res, y, X, geno, map=bim, message=msgs.append)
    names = ["rs%04d" % (1000 + j) for j in res["selected_loci"]]
    assert got["pvalue"]["effects"] == ["intercept"] + names and got["R"]["Marker_name"] == ["+ " + nm for nm in names]
    printed = "\n".join(str(m) for m in msgs)
    assert all(nm in printed for nm in names) and "rs1021" in printed and "rs1071" in printed
    rcpp_api.drop_cache()
