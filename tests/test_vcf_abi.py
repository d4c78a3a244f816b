"""CPU: the C ABI of the VCF ingestion without a device -- eagle_vcf_to_bed is declared, exported and bound, section 1b-vcf of the header
states the rule and what is not claimed, and every argument error is decided before a context is needed (ctx == NULL: the text comes
through eagle_open_error).  The HIP-free pieces behind it (csrc/eagle_host.h: the line splitter of a staged window, the header line,
the fixed-field parser and the verdict on a data line) also run in a stand-alone program under ASan + UBSan, built as
tests/test_roh_abi.py builds its neighbour; nothing is preloaded.  No device work."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT

ERR_ARG = -3
COUNT_FIELDS = ("lines", "kept", "multiallelic", "no_alt", "no_gt", "not_snp", "filtered", "missing", "haploid", "malformed")


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_vcf_symbol_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    assert re.search(r"\bint\s+eagle_vcf_to_bed\s*\(\s*eagle_ctx\s*\*", txt), "eagle_vcf_to_bed is not declared in include/eagle_hip.h"
    assert hasattr(L, "eagle_vcf_to_bed"), "libeaglehip.so does not export eagle_vcf_to_bed"
    res, args = _lib.SIGNATURES["eagle_vcf_to_bed"]
    assert res is C.c_int and len(args) == 8 and args[3] is C.c_int and args[4] is C.c_double and args[5] is C.c_long
    m = re.search(r"typedef struct eagle_vcf_counts \{\s*long ([^;]*);", txt)
    assert m and tuple(f.strip() for f in m.group(1).split(",")) == tuple(f for f, _ in _lib.VcfCounts._fields_) == COUNT_FIELDS
    assert C.sizeof(_lib.VcfCounts) == 10 * C.sizeof(C.c_long) and rcpp_api.VCF_COUNT_FIELDS == COUNT_FIELDS
    for name, value in (("EAGLE_VCF_A2_ALT", 1), ("EAGLE_VCF_SNPS_ONLY", 2), ("EAGLE_VCF_PASS_ONLY", 4)):
        assert re.search(r"#define %s %d\b" % (name, value), txt)
    assert (rcpp_api.VCF_A2_ALT, rcpp_api.VCF_SNPS_ONLY, rcpp_api.VCF_PASS_ONLY) == (1, 2, 4)
    ctxh = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ctx.h")).read()
    for name in ("eagle_dev_vcf_fields", "eagle_dev_vcf_pack"):
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, ctxh) and hasattr(L, name)
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_vcf.hip" in makefile and "eagle_vcf.o" in makefile
    kern = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_vcf.hip")).read()
    assert "k_vcf_fields" in kern and "k_vcf_pack" in kern and "asm" not in re.sub(r"//.*", "", kern)
    code = re.sub(r"//.*", "", kern)
    assert "double" not in code and "float" not in code                                      # integer work only


def test_header_states_the_rule_and_what_is_not_claimed():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b-vcf."):txt.index("1b'. Marker QC")]
    for phrase in ("neither claimed nor tested", "Sex chromosomes, dosages (DS / GP), phase and the splitting of multi-allelic records are out of scope",
                   "a '\\r' before the '\\n' is dropped", "an unterminated last line is a line", "empty lines are skipped anywhere",
                   "Line numbers are 1-based", 'Lines that start with "##" are skipped', 'must start with "#CHROM"',
                   "from the 10th on are the n sample names", "fewer than 10 columns", "a sample name that is empty or contains a blank",
                   "a data line before the header", "from the nine fixed fields alone", "under the FIRST reason that holds",
                   "ALT contains a ',' (multiallelic)", 'ALT is "." (no_alt)', 'FORMAT is not "GT" and does not begin with "GT:" (no_gt)',
                   "REF or ALT is not one of A C G T, case-insensitive (not_snp)", 'FILTER is neither "PASS" nor "." (filtered)',
                   "exactly n sample fields", "naming the line and the count found", "the bytes up to the next tab or the line end",
                   "GT is the field up to its first ':'", "bytes after the first ':' are never looked at", "cut at every '/' or '|' into k tokens",
                   'k = 1, token "0" -> homozygous REF, counted haploid', 'k = 1, token "1" -> homozygous ALT, counted haploid',
                   'k = 2, both tokens in {"0", "1"}', "different -> het", "anything else -> missing",
                   'whose tokens are not all "." is also counted malformed', '"2/1", "10/1", "0/1/1"', "an empty field, an empty token",
                   "00 hom A1, 10 het, 01 missing, 11 hom A2", "the unused bit pairs of a row's last byte zero", "By default A1 = ALT and A2 = REF",
                   "EAGLE_VCF_A2_ALT makes A2 = ALT", "CHROM \\t ID \\t 0 \\t POS \\t A1 \\t A2", 'ID = CHROM:POS where the file has "."',
                   '"name name 0 0 0 -9"', "A failed call leaves none of the three files", "A window holds whole lines only",
                   "grows to the longest line", "is EAGLE_ERR_ARG", "The pread of window k runs under the device work of window k - 1",
                   "write-behind", "the same file gives the same bytes at every value", "decided before the context is used",
                   "a NULL pointer, unknown flag bits, chunk_bytes < 0, an empty prefix", "works on its first device"):
        assert phrase in sec, phrase
    assert txt.index("1b. Marker-file ingestion") < txt.index("1b-vcf.") < txt.index("1b'. Marker QC")
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "VCF" in readme and "Agreement with PLINK or bcftools is neither claimed nor tested" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.8" in design and "eagle_vcf_to_bed" in design


def test_vcf_interface_is_public():
    import eagleeverything_amd
    from eagleeverything_amd import r_api, rcpp_api
    p = inspect.signature(rcpp_api.vcf_to_bed).parameters
    assert [(k, v.default) for k, v in p.items()][2:] == [("a2", "ref"), ("snps_only", False), ("pass_only", False), ("availmemGb", 8),
                                                          ("chunk_bytes", 0), ("device", 0)]
    assert list(p)[:2] == ["vcf", "out_prefix"] and list(inspect.signature(r_api.VcfToBed).parameters) == list(p)
    assert list(inspect.signature(r_api.vcf_to_bed_host).parameters) == ["vcf_bytes", "a2", "snps_only", "pass_only"]
    assert "VCF" in eagleeverything_amd.__doc__
    said = []
    assert r_api.ReadMarker("/nonexistent/x.vcf", type="VCF", message=said.append) is None and "could not be found" in said[0]
    said = []
    assert r_api.ReadMarker("/nonexistent/x.vcf", type="vcf", message=said.append) is None
    assert said[0] == ' type must be set to "text" or "PLINK". \n'
    with pytest.raises(ValueError):
        rcpp_api.vcf_flags(a2="A1")
    assert rcpp_api.vcf_flags("alt", True, True) == 7 and rcpp_api.vcf_flags() == 0


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()

    dims, counts = (C.c_long * 2)(), _lib.VcfCounts()
    good = (str(tmp_path / "a.vcf").encode(), str(tmp_path / "out").encode(), 0, 8.0, 0, dims, C.byref(counts))
    names = ("vcf", "prefix", "flags", "mem", "chunk", "dims", "counts")

    def call(**kw):
        return L.eagle_vcf_to_bed(None, *[kw.get(k, v) for k, v in zip(names, good)])
    for k in ("vcf", "prefix", "dims", "counts"):
        assert call(**{k: None}) == ERR_ARG and text().startswith("vcf_to_bed:") and "NULL" in text(), k
    assert call(flags=8) == ERR_ARG and "unknown flag bits" in text() and "1b-vcf" in text()
    assert call(flags=-1) == ERR_ARG and "unknown flag bits" in text()
    assert call(chunk=-1) == ERR_ARG and "chunk_bytes" in text()
    assert call(chunk=(1 << 30) + 1) == ERR_ARG and "chunk_bytes" in text()
    assert call(prefix=b"") == ERR_ARG and "empty output prefix" in text()
    # what passes the rule stops at the missing context, and nothing was written
    for kw in ({}, dict(flags=7), dict(chunk=1), dict(chunk=1 << 30), dict(mem=0.0)):
        assert call(**kw) == ERR_ARG and "no context" in text()
    assert os.listdir(tmp_path) == []


def test_vcf_host_pieces_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "vcf_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_vcf_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "vcf host checks passed" in r.stdout
