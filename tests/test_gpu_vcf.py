"""VCF ingestion on the GPU: eagle_vcf_to_bed / r_api.VcfToBed / ReadMarker(type="VCF") (k_vcf_fields and k_vcf_pack on the hot path).

The device's three files are compared with r_api.vcf_to_bed_host's -- the rule of include/eagle_hip.h section 1b-vcf restated in plain
Python, itself held to hand-written bytes by tests/test_vcf_host.py -- byte for byte, and the counts with ==.  No tolerance anywhere.
Every file is converted at chunk_bytes = 1 (one line a window, grown to the line), at a value that holds two to three lines, and at 0:
all three must leave the same bytes."""
import gzip
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN

TINY = os.path.join(GOLDEN, "vcf", "tiny.vcf")
ERR_FORMAT = -2
HEADER9 = [b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO", b"FORMAT"]
GTS = [b"0/0", b"0/1", b"1/1", b"0|1", b"1|0", b"1|1", b"0|0", b"./.", b".|.", b".", b"0", b"1"]       # drawn often
ODD = [b"2/1", b"10/1", b"0/1/1", b"", b"/1", b"1/", b"./1", b"0/.", b"a", b"01", b"0/1/", b"..", b"./././."]    # drawn rarely
TAILS = [b"", b"", b":7", b":0:0,0,0", b":23:11,12:0/1|.:99,0,255", b":.:.:1|0:./.:0/0:1/1:.,.,.:" + b"8" * 37]
SEG = 4096


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def make_vcf(n, seed, lines=40):
    """A VCF of n samples and `lines` data lines, some of them dropped ones, with fields of random width -- so that field starts, and
    GTs that straddle a boundary, fall on every residue of 16 -- and, in lines longer than one 4,096-byte segment, a GT planted in the
    last byte of the first segment as k_vcf_fields cuts the line when it starts a window (chunk_bytes = 1)."""
    rng = np.random.default_rng(seed)
    out = [b"##fileformat=VCFv4.2", b"##made for tests/test_gpu_vcf.py", b"\t".join(HEADER9 + [b"s%d" % i for i in range(n)]), b""]
    for m in range(lines):
        kind = ("keep", "keep", "keep", "keep", "keep", "keep", "multi", "noalt", "nogt", "keep")[m % 10]
        ref, alt, fmt = b"A", b"C", (b"GT", b"GT:DP", b"GT:AD:DP:GQ:PL")[m % 3]
        if kind == "multi":
            alt = b"C,G"
        elif kind == "noalt":
            alt = b"."
        elif kind == "nogt":
            fmt = b"DP:GT"
        vid = b"." if m % 4 == 0 else b"rs%d" % (1000 + m)
        fixed = b"\t".join([b"%d" % (1 + m // 17), b"%d" % (100 + 13 * m), vid, ref, alt, b"%d" % (m % 60), (b"PASS", b".", b"q10")[m % 3],
                            b"DP=%d;AF=0.5" % m, fmt]) + b"\t"
        nf = n if kind == "keep" or m % 20 < 10 else max(1, n // 3)        # the sample fields of a dropped line are never looked at
        g = rng.integers(0, len(GTS), size=nf)
        odd = rng.random(nf) < 0.04
        o = rng.integers(0, len(ODD), size=nf)
        t = rng.integers(0, len(TAILS), size=nf)
        fields = [(ODD[o[i]] if odd[i] else GTS[g[i]]) + TAILS[t[i]] for i in range(nf)]
        if kind == "keep" and m % 2 == 0:
            # the planted GT: field j starts at the last byte of the first segment, the field before it is lengthened behind its ':'
            target = (len(fixed) & ~15) + SEG - 1
            at, j = len(fixed), 0
            while j < nf and at + len(fields[j]) + 1 < target - 8:
                at += len(fields[j]) + 1
                j += 1
            if 0 < j < nf - 1 and at < target:
                fields[j] = fields[j].split(b":")[0] + b":" + b"5" * (target - at - len(fields[j].split(b":")[0]) - 2)
                assert at + len(fields[j]) + 1 == target
                fields[j + 1] = (b"0/1", b"1|1:3", b"./.", b"0")[m // 2 % 4]
        out.append(fixed + b"\t".join(fields))
        if m % 7 == 3:
            out.append(b"")
    text = b"\n".join(out)
    if seed % 2:
        text = text.replace(b"\n", b"\r\n")
    return text if seed % 3 == 0 else text + b"\n"                          # every third file ends without a newline


def host(text, **kw):
    from eagleeverything_amd import r_api
    return r_api.vcf_to_bed_host(text, **kw)


def convert_and_compare(tmp_path, text, want, chunks, **kw):
    from eagleeverything_amd import r_api
    bed, bim, fam, dims, counts = want
    src = str(tmp_path / "in.vcf")
    with open(src, "wb") as f:
        f.write(text)
    for c in chunks:
        res = r_api.VcfToBed(src, str(tmp_path / ("out_%d" % c) / "panel"), chunk_bytes=c, **kw)
        assert res["dims"] == dims and res["counts"] == counts, c
        assert _read(res["bed"]) == bed, c
        assert _read(res["bim"]).decode("latin-1") == bim and _read(res["fam"]).decode("latin-1") == fam, c
        assert res["samples"] == [ln.split()[0] for ln in fam.splitlines()]
        shutil.rmtree(str(tmp_path / ("out_%d" % c)))


# last-byte padding; wave edges; workgroup edges; one line longer than one 4,096-byte segment; several segments
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099])
def test_gpu_vcf_files_equal_the_host_restatement_at_every_window_size(tmp_path, n):
    text = make_vcf(n, seed=n)
    longest = max(len(ln) for ln in text.split(b"\n")) + 1
    if n >= 1023:
        assert longest > SEG + 64 and (n < 4099 or longest > 4 * SEG)
    a2 = "alt" if n % 2 else "ref"
    want = host(text, a2=a2)
    assert want[3][0] == n and 20 <= want[3][1] < 40 and want[4]["missing"] > 0 and want[4]["haploid"] > 0
    assert n < 63 or want[4]["malformed"] > 0
    convert_and_compare(tmp_path, text, want, (1, int(2.5 * longest), 0), a2=a2)


@pytest.mark.gpu
def test_gpu_vcf_tiny_fixture_and_flags(tmp_path):
    text = _read(TINY)
    for i, kw in enumerate((dict(), dict(a2="alt"), dict(snps_only=True), dict(pass_only=True), dict(a2="alt", snps_only=True, pass_only=True))):
        sub = tmp_path / ("f%d" % i)
        sub.mkdir()
        convert_and_compare(sub, text, host(text, **kw), (1, 200, 0), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 300])
def test_gpu_vcf_wrong_field_count_names_the_line_and_leaves_no_files(tmp_path, n):
    from eagleeverything_amd import rcpp_api
    from eagleeverything_amd._lib import EagleError
    lines = make_vcf(n, seed=7 + n).replace(b"\r\n", b"\n").split(b"\n")
    kept = [i for i, ln in enumerate(lines) if ln and not ln.startswith(b"#") and b"\tC\t" in ln and b"\tDP:GT\t" not in ln]
    for which, delta, c in ((kept[0], -1, 0), (kept[5], +1, 1), (kept[-1], -1, 3000), (kept[9], +1, 0)):
        bad = list(lines)
        f = bad[which].split(b"\t")
        bad[which] = b"\t".join(f[:-1] if delta < 0 else f + [b"0/0"])
        src, prefix = str(tmp_path / "bad.vcf"), str(tmp_path / "bad_out")
        with open(src, "wb") as fh:
            fh.write(b"\n".join(bad))
        with pytest.raises(ValueError) as he:
            host(b"\n".join(bad))
        assert "line %d: %d sample fields" % (which + 1, n + delta) in str(he.value)
        with pytest.raises(EagleError) as e:
            rcpp_api.vcf_to_bed(src, prefix, chunk_bytes=c)
        assert e.value.code == ERR_FORMAT and "line %d: %d sample fields" % (which + 1, n + delta) in e.value.text and "1b-vcf" in e.value.text
        assert [p for p in os.listdir(tmp_path) if p.startswith("bad_out")] == []
    for data, line, words in ((b"##x\n\n" + lines[5] + b"\n", 3, "#CHROM"), (b"##x\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\n", 2, "10 columns")):
        src = str(tmp_path / "hdr.vcf")
        with open(src, "wb") as fh:
            fh.write(data)
        with pytest.raises(EagleError) as e:
            rcpp_api.vcf_to_bed(src, str(tmp_path / "bad_out"))
        assert e.value.code == ERR_FORMAT and ("line %d:" % line) in e.value.text and words in e.value.text
        assert [p for p in os.listdir(tmp_path) if p.startswith("bad_out")] == []


@pytest.mark.gpu
def test_gpu_read_marker_vcf_equals_the_bed_route(tmp_path):
    from eagleeverything_amd import r_api
    text = make_vcf(150, seed=150)
    bed, bim, fam, dims, counts = host(text)
    n, L = dims
    codes = np.frombuffer(bed, dtype=np.uint8)[3:].reshape(L, -1)
    codes = np.stack([(codes >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(L, -1)[:, :n]
    src = str(tmp_path / "panel150.vcf")
    with open(src, "wb") as f:
        f.write(text)
    geno = r_api.ReadMarker(src, type="VCF", outdir=str(tmp_path / "a"))
    assert geno["dim_of_ascii_M"] == [n, L] and geno["vcf_counts"] == counts and geno["samples"] == ["s%d" % i for i in range(n)]
    assert geno["bed"] == str(tmp_path / "a" / "vcf" / "panel") and _read(geno["bed"] + ".bed") == bed
    stats = r_api.MarkerStats(geno, bed=geno["bed"])
    for key, code in (("n0", 0), ("n1", 2), ("n2", 3), ("n_missing", 1)):
        assert np.array_equal(np.asarray(stats[key]), (codes == code).sum(axis=1)), key
    # the host restatement's fileset through the .bed route: the same M.ascii and Mt.ascii
    ref_prefix = str(tmp_path / "ref" / "panel")
    os.makedirs(os.path.dirname(ref_prefix))
    for ext, blob in ((".bed", bed), (".bim", bim.encode("latin-1")), (".fam", fam.encode("latin-1"))):
        with open(ref_prefix + ext, "wb") as f:
            f.write(blob)
    ref = r_api.ReadMarker(ref_prefix, type="PLINKbed", outdir=str(tmp_path / "ref"))
    assert _read(geno["asciifileM"]) == _read(ref["asciifileM"]) and _read(geno["asciifileMt"]) == _read(ref["asciifileMt"])
    assert ref["dim_of_ascii_M"] == [n, L]


@pytest.mark.gpu
def test_gpu_read_marker_gzip_equals_the_plain_file(tmp_path):
    from eagleeverything_amd import r_api
    plain = r_api.ReadMarker(TINY, type="VCF", outdir=str(tmp_path / "plain"))
    gz = str(tmp_path / "tiny.vcf.gz")
    data = _read(TINY)
    with open(gz, "wb") as f:                                               # two members, as bgzip writes many
        f.write(gzip.compress(data[:200]) + gzip.compress(data[200:]))
    packed = r_api.ReadMarker(gz, type="VCF", outdir=str(tmp_path / "gz"))
    assert plain["dim_of_ascii_M"] == packed["dim_of_ascii_M"] == [5, 5] and plain["vcf_counts"] == packed["vcf_counts"]
    for ext in (".bed", ".bim", ".fam"):
        assert _read(plain["bed"] + ext) == _read(packed["bed"] + ext)
    assert _read(plain["asciifileM"]) == _read(packed["asciifileM"]) and _read(plain["asciifileMt"]) == _read(packed["asciifileMt"])
    assert sorted(os.listdir(str(tmp_path / "gz" / "vcf"))) == ["panel.bed", "panel.bim", "panel.fam"]      # the inflated copy is gone
    assert _read(plain["bed"] + ".bed") == host(data)[0]
