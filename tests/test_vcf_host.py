"""CPU: r_api.vcf_to_bed_host, the restatement of include/eagle_hip.h section 1b-vcf in plain Python and numpy, held to expectations
written by hand for tests/golden/vcf/tiny.vcf (13 lines, 5 samples: every GT form of the rule's table, every drop reason, a CRLF line,
empty lines, an unterminated last line, a FORMAT of GT alone, subfields behind the ':' that hold 0 1 / | .), to every FORMAT error with
its line number, and to a round trip through read_bed_codes.  tests/test_gpu_vcf.py compares the device's files with this function's."""
import os

import numpy as np
import pytest

from conftest import ROOT

TINY = os.path.join(ROOT, "tests", "golden", "vcf", "tiny.vcf")
HEAD = b"\x6c\x1b\x01"
FAM = "".join("S%d S%d 0 0 0 -9\n" % (i, i) for i in range(1, 6))
# kept by default: lines 5, 6, 11, 12, 13 of the file.  Codes with A1 = ALT: hom REF 3, het 2, hom ALT 0, missing 1; 5 samples = 2 bytes a row.
#   line 5   0/0 0/1 1/1 ./. 1|0                  -> 3 2 0 1 2 -> 0x4b 0x02
#   line 6   0|0:.. 1:.. 0:.. .:.. 1/0:..  (CRLF) -> 3 0 3 1 2 -> 0x73 0x02    two haploid calls, "." missing and not malformed
#   line 11  2/1 10/1 0/1/1 <empty> /1            -> 1 1 1 1 1 -> 0x55 0x01    five malformed
#   line 12  0/0:1 1/1:0|1 0/1:./. ./.:1 .|.:0/0  -> 3 0 2 1 1 -> 0x63 0x01
#   line 13  1/1 1|1 0|1 ./1 .   (no newline)     -> 0 0 2 1 1 -> 0x60 0x01    ./1 malformed
BED_REF = HEAD + bytes([0x4b, 0x02, 0x73, 0x02, 0x55, 0x01, 0x63, 0x01, 0x60, 0x01])
BED_ALT = HEAD + bytes([0x78, 0x02, 0x4c, 0x02, 0x55, 0x01, 0x6c, 0x01, 0x6f, 0x01])       # hom REF 0, hom ALT 3
BIM_REF = "1\trs1\t0\t100\tC\tA\n1\t1:200\t0\t200\tT\tG\n2\trs6\t0\t600\tA\tAT\n2\trs7\t0\t700\tt\ta\n2\t2:800\t0\t800\tG\tC\n"
BIM_ALT = "1\trs1\t0\t100\tA\tC\n1\t1:200\t0\t200\tG\tT\n2\trs6\t0\t600\tAT\tA\n2\trs7\t0\t700\ta\tt\n2\t2:800\t0\t800\tC\tG\n"
COUNTS = dict(lines=8, kept=5, multiallelic=1, no_alt=1, no_gt=1, not_snp=0, filtered=0, missing=11, haploid=2, malformed=6)


def tiny():
    return open(TINY, "rb").read()


def test_fixture_is_what_the_expectations_assume():
    data = tiny()
    assert len(data) < 4096 and not data.endswith(b"\n") and data.count(b"\r\n") == 1 and b"\n\n" in data
    assert data.split(b"\n")[4].split(b"\t")[8] == b"GT" and data.split(b"\n")[5].split(b"\t")[8] == b"GT:DP:AD"


def test_tiny_default_a2_is_ref():
    from eagleeverything_amd import r_api
    bed, bim, fam, dims, counts = r_api.vcf_to_bed_host(tiny())
    assert bed == BED_REF and bim == BIM_REF and fam == FAM and dims == [5, 5] and counts == COUNTS


def test_tiny_a2_alt():
    from eagleeverything_amd import r_api
    bed, bim, fam, dims, counts = r_api.vcf_to_bed_host(tiny(), a2="alt")
    assert bed == BED_ALT and bim == BIM_ALT and fam == FAM and dims == [5, 5] and counts == COUNTS


def test_tiny_snps_only_and_pass_only():
    from eagleeverything_amd import r_api
    bed, bim, _, dims, counts = r_api.vcf_to_bed_host(tiny(), snps_only=True)          # line 11: REF = AT; line 12's a / t are bases
    assert bed == BED_REF[:7] + BED_REF[9:] and bim == "".join(BIM_REF.splitlines(True)[i] for i in (0, 1, 3, 4)) and dims == [5, 4]
    assert counts == dict(COUNTS, kept=4, not_snp=1, missing=6, malformed=1)
    bed, bim, _, dims, counts = r_api.vcf_to_bed_host(tiny(), pass_only=True)          # line 12: FILTER = q10; line 13's "." passes
    assert bed == BED_REF[:9] + BED_REF[11:] and bim == "".join(BIM_REF.splitlines(True)[i] for i in (0, 1, 2, 4)) and dims == [5, 4]
    assert counts == dict(COUNTS, kept=4, filtered=1, missing=9)
    bed, _, _, dims, counts = r_api.vcf_to_bed_host(tiny(), a2="alt", snps_only=True, pass_only=True)
    assert bed == BED_ALT[:7] + BED_ALT[11:] and dims == [5, 3]
    assert counts == dict(COUNTS, kept=3, not_snp=1, filtered=1, missing=4, malformed=1)


def test_line_ends_do_not_matter():
    from eagleeverything_amd import r_api
    want = r_api.vcf_to_bed_host(tiny())
    unix = tiny().replace(b"\r\n", b"\n")
    assert r_api.vcf_to_bed_host(unix) == want and r_api.vcf_to_bed_host(unix + b"\n") == want
    assert r_api.vcf_to_bed_host(unix.replace(b"\n", b"\r\n")) == want and r_api.vcf_to_bed_host(unix + b"\n\n\r\n") == want


HDR = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\tC\n"
ROW = b"1\t%d\t.\tA\tC\t.\t.\t.\tGT\t"


@pytest.mark.parametrize("data, line, words", [
    (b"##x\n\n1\t5\t.\tA\tC\t.\t.\t.\tGT\t0/0\n" + HDR, 3, "#CHROM"),                            # a data line before the header
    (b"##x\n##y\n", 3, "#CHROM"),                                                                    # no header at all
    (b"##x\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\n", 2, "fewer than 10 columns"),
    (b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n", 1, "fewer than 10 columns"),
    (b"##x\n\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\t\tC\n", 3, "sample name"),
    (b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\t\n", 1, "sample name"),
    (b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB b\tC\n", 1, "sample name"),
    (HDR + ROW % 1 + b"0/0\t0/1\t1/1\n" + ROW % 2 + b"0/0\t0/1\n", 4, "2 sample fields"),
    (HDR + ROW % 1 + b"0/0\t0/1\t1/1\n\n" + ROW % 2 + b"0/0\t0/1\t1/1\t./.\r\n", 5, "4 sample fields"),
    (HDR + ROW % 1 + b"0/0\t0/1\t1/1\n" + (ROW % 2)[:-1] + b"\n", 4, "0 sample fields"),
    (HDR + b"1\t7\t.\tA\tC\t.\t.\t.\n", 3, "fewer than nine"),
])
def test_format_errors_name_the_line(data, line, words):
    from eagleeverything_amd import r_api
    with pytest.raises(ValueError) as e:
        r_api.vcf_to_bed_host(data)
    assert ("line %d:" % line) in str(e.value) and words in str(e.value)


def test_dropped_lines_are_not_looked_at_and_nothing_kept_is_an_error():
    from eagleeverything_amd import r_api
    ok = HDR + ROW % 1 + b"0/0\t0/1\t1/1\n" + b"1\t2\t.\tA\tC,T\t.\t.\t.\tGT\t0/0\n"         # the dropped line has one sample field
    bed, _, _, dims, counts = r_api.vcf_to_bed_host(ok)
    assert dims == [3, 1] and counts["multiallelic"] == 1 and bed == HEAD + bytes([3 | 2 << 2])
    with pytest.raises(ValueError):
        r_api.vcf_to_bed_host(HDR + b"1\t2\t.\tA\t.\t.\t.\t.\tGT\t0/0\t0/0\t0/0\n")
    with pytest.raises(ValueError):
        r_api.vcf_to_bed_host(tiny(), a2="A2")


def test_round_trip_through_read_bed_codes(tmp_path):
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(28)
    L, n = 37, 23
    codes = rng.integers(0, 4, size=(L, n)).astype(np.uint8)
    for a2, text in (("ref", {3: b"0/0", 2: b"0|1", 0: b"1/1", 1: b"./."}), ("alt", {0: b"0/0", 2: b"1/0", 3: b"1|1", 1: b"."})):
        out = [b"##fileformat=VCFv4.2", b"\t".join([b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO", b"FORMAT"] +
                                                    [b"i%d" % i for i in range(n)])]
        for m in range(L):
            out.append(b"\t".join([b"3", b"%d" % (10 * m + 1), b"m%d" % m, b"G", b"A", b".", b"PASS", b".", b"GT:DP"] +
                                  [text[int(c)] + b":%d" % (i % 11) for i, c in enumerate(codes[m])]))
        bed, bim, fam, dims, counts = r_api.vcf_to_bed_host(b"\n".join(out) + b"\n", a2=a2)
        assert dims == [n, L] and counts["kept"] == L == counts["lines"] and counts["missing"] == int((codes == 1).sum())
        assert counts["malformed"] == 0 and counts["haploid"] == 0
        prefix = str(tmp_path / ("rt_" + a2))
        for ext, blob in ((".bed", bed), (".bim", bim.encode()), (".fam", fam.encode())):
            with open(prefix + ext, "wb") as f:
                f.write(blob)
        assert np.array_equal(r_api.read_bed_codes(prefix, dims), codes)
        assert r_api.ReadBim(prefix + ".bim")["Pos"] == [10 * m + 1 for m in range(L)] and len(fam.splitlines()) == n
