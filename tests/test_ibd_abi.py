"""CPU: the C ABI of the pairwise IBD-type segments without a device -- eagle_ibd and eagle_bed_ibd are declared, exported and bound,
section 1b'''vii of the header states the rule and what is not claimed, and every argument error of rule 10 is decided before a context is
needed (ctx == NULL: the text comes through eagle_open_error).  The HIP-free pieces behind them (csrc/eagle_host.h: ibd_arg_error,
ibd_pairs_check, ibd_offsets, ibd_cut_plane, ...) also run in a stand-alone program under ASan + UBSan, built as tests/test_roh_abi.py
builds its source.  No device work."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
NAMES = ("eagle_ibd", "eagle_bed_ibd")


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_ibd_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    assert len(_lib.SIGNATURES["eagle_ibd"][1]) == 13 and len(_lib.SIGNATURES["eagle_bed_ibd"][1]) == 14
    m = re.search(r"typedef struct eagle_ibd_params \{\s*int64_t ([^;]*);", txt)
    assert m and tuple(f.strip() for f in m.group(1).split(",")) == tuple(f for f, _ in _lib.IbdParams._fields_) == rcpp_api._IBD_FIELDS
    assert C.sizeof(_lib.IbdParams) == 40
    assert re.search(r"#define EAGLE_IBD_MAX_PAIRS 134217728L", txt) and rcpp_api.IBD_MAX_PAIRS == 134217728
    ctxh = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ctx.h")).read()
    for name in ("eagle_dev_ibd_planes_i8", "eagle_dev_ibd_planes_bed", "eagle_dev_ibd_walk"):
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, ctxh) and hasattr(L, name)
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_ibd.hip" in makefile and "eagle_ibd.o" in makefile
    kern = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ibd.hip")).read()
    assert "k_ibd_planes_i8" in kern and "k_ibd_planes_bed" in kern and "k_ibd_walk" in kern and "asm" not in re.sub(r"//.*", "", kern)


def test_header_states_the_rule_and_what_is_not_claimed():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b'''vii."):txt.index("1b''''.")]
    for phrase in ("IBIS or TRUFFLE programs is neither claimed nor tested", "bound IBD from above", "a missing call of the original data is a het",
                   "code 01 is not called", "g_i g_j = -1, opposite homozygotes", "g_i != g_j", "either is not called is never a break",
                   "NULL: pos[m] = m", "non-decreasing inside every block", "pos[m + 1] - pos[m] > max_gap", "PIECES",
                   "maximal sequence of consecutive non-break markers inside one piece", "merge_min = 0 every pure run is a candidate on its own",
                   "ELIGIBLE iff it has at least merge_min markers", "separated by exactly one marker (a single break)",
                   "An ineligible run is a chain of its own", "two breaks in a row, or a cut, end a chain", "do not depend on the walking order",
                   "nsnp = e - s + 1 >= min_snp", "len = pos[e] - pos[s] >= min_len", "nbreak = k - 1", "0 <= i < j < n, duplicates allowed",
                   "k = i n - i (i + 1) / 2 + (j - i - 1)", "P x 4 int64", "(i, j, s, e, nbreak, block ordinal)", "sorted by (pair ordinal, s)",
                   "nseg_out is always the total", "untouched otherwise", "returns EAGLE_OK either way", "n <= 0x3fffffff",
                   "EAGLE_ERR_NOMEM, decided before any kernel runs", "does not depend on the window size", "decided before the context is used",
                   "no array of pairs x markers exists"):
        assert phrase in sec, phrase
    assert txt.index("1b'''vi.") < txt.index("1b'''vii.") < txt.index("1b''''.")
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "Pairwise IBD segments" in readme and "IBIS or TRUFFLE programs is neither claimed nor tested" in readme


def test_ibd_interface_is_public():
    from eagleeverything_amd import r_api, rcpp_api
    for name in ("ibd_host", "ibd_genotypes_bed", "ibd_all_pairs", "ibd_incidence", "ibd_summary", "ibd_kinship", "IBD"):
        assert callable(getattr(r_api, name))
    p = inspect.signature(r_api.IBD).parameters
    assert [(k, p[k].default) for k in list(p)[1:11]] == [
        ("map", None), ("bed", None), ("include", None), ("pairs", None), ("mode", "ibs1"), ("min_snp", 200), ("min_kb", 1000),
        ("max_gap_kb", 1000), ("merge_min_snp", 100), ("availmemGb", 8)]
    assert list(inspect.signature(r_api.ibd_host).parameters) == ["g", "called", "pairs", "chrom", "pos", "params"]
    assert list(inspect.signature(r_api.ibd_kinship).parameters) == ["ibs1", "ibs2"]
    p = inspect.signature(rcpp_api.ibd).parameters
    assert list(p)[:5] == ["f_name_ascii_M", "dims", "pairs", "chrom", "pos"] and all(p[k].default is None for k in ("pairs", "chrom", "pos"))
    p = inspect.signature(rcpp_api.bed_ibd).parameters
    assert list(p)[:6] == ["bed_path", "dims", "include", "pairs", "chrom", "pos"] and p["include"].default is None
    assert rcpp_api.IBD_DEFAULTS == dict(mode=1, min_snp=200, min_len=0, max_gap=0, merge_min=100)
    assert rcpp_api.ibd_params(mode="ibs2")["mode"] == 2 and rcpp_api.ibd_params(mode="ibs1", merge_min=0)["merge_min"] == 0
    doc = " ".join(r_api.IBD.__doc__.split()) + " ".join(r_api.ibd_kinship.__doc__.split())
    for phrase in ("bound IBD from above", "INFLATE mode \"ibs1\"", "CUT mode \"ibs2\"", "route for un-imputed panels", "k1 / 4 + k2 / 2"):
        assert phrase in doc, phrase


def params(**kw):
    from eagleeverything_amd import _lib, rcpp_api
    p = dict(rcpp_api.IBD_DEFAULTS)
    p.update(kw)
    return _lib.IbdParams(*[p[f] for f in rcpp_api._IBD_FIELDS])


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()

    nm, n = 7, 5
    dims = (C.c_long * 2)(n, nm)
    tab, seg, total = (C.c_int64 * (4 * 10))(), (C.c_int32 * (6 * 8))(), C.c_long(0)
    chrom, pos = (C.c_int32 * nm)(1, 1, 1, 2, 2, 3, 3), (C.c_int64 * nm)(10, 20, 30, 5, 6, 1, 1)
    plist = (C.c_int32 * 6)(0, 1, 0, 1, 3, 4)

    def ref(p):
        return C.cast(C.pointer(p), C.c_void_p)

    for fn, who, good, names in (
            (L.eagle_ibd, "ibd", (str(tmp_path / "M.ascii").encode(), dims, None, 0, chrom, pos, ref(params()), 8.0, tab, seg, 8, C.byref(total)),
             ("path", "dims", "pairs", "npairs", "chrom", "pos", "prm", "mem", "tab", "seg", "cap", "total")),
            (L.eagle_bed_ibd, "bed_ibd",
             (str(tmp_path / "p.bed").encode(), dims, None, None, 0, chrom, pos, ref(params()), 8.0, tab, seg, 8, C.byref(total)),
             ("path", "dims", "include", "pairs", "npairs", "chrom", "pos", "prm", "mem", "tab", "seg", "cap", "total"))):

        def call(**kw):
            return fn(None, *[kw.get(k, v) for k, v in zip(names, good)])
        assert call(path=None) == ERR_ARG and text().startswith(who + ":") and "NULL" in text()
        assert call(dims=None) == ERR_ARG and "NULL" in text()
        assert call(prm=None) == ERR_ARG and "NULL" in text()
        assert call(tab=None) == ERR_ARG and "NULL" in text()
        assert call(total=None) == ERR_ARG and "NULL" in text()
        assert call(seg=None) == ERR_ARG and "seg_out" in text()                        # seg_cap > 0 needs the buffer
        assert call(cap=-1) == ERR_ARG and "seg_cap" in text()
        assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
        assert call(dims=(C.c_long * 2)(n, -1)) == ERR_ARG and "dims" in text()
        assert call(dims=(C.c_long * 2)(n, 1 << 31), chrom=None, pos=None) == ERR_ARG and "2^31" in text()
        for kw, word in ((dict(mode=0), "mode must be 1 (ibs1) or 2 (ibs2)"), (dict(mode=3), "mode must be"), (dict(min_snp=0), "min_snp"),
                         (dict(min_len=-1), "min_len"), (dict(max_gap=-1), "max_gap"), (dict(merge_min=-1), "merge_min")):
            assert call(prm=ref(params(**kw))) == ERR_ARG and word in text() and text().startswith(who + ":"), kw
        # pairs: a list of 1 .. 2^27 entries with 0 <= i < j < n; all pairs need 2 <= n and n (n - 1) / 2 <= 2^27
        assert call(pairs=plist, npairs=0) == ERR_ARG and "number of pairs" in text()
        assert call(pairs=plist, npairs=-1) == ERR_ARG and "number of pairs" in text()
        assert call(pairs=plist, npairs=(1 << 27) + 1) == ERR_ARG and "number of pairs" in text()
        assert call(pairs=(C.c_int32 * 6)(0, 1, 2, 2, 3, 4), npairs=3) == ERR_ARG and "pair 1 is not 0 <= i < j < n" in text()
        assert call(pairs=(C.c_int32 * 6)(0, 1, 0, 1, 4, 3), npairs=3) == ERR_ARG and "pair 2" in text()
        assert call(pairs=(C.c_int32 * 6)(-1, 1, 0, 1, 3, 4), npairs=3) == ERR_ARG and "pair 0" in text()
        assert call(pairs=(C.c_int32 * 6)(0, 1, 0, 1, 3, 5), npairs=3) == ERR_ARG and "pair 2" in text()
        assert call(dims=(C.c_long * 2)(1, nm)) == ERR_ARG and "two individuals" in text()
        assert call(dims=(C.c_long * 2)(16385, nm)) == ERR_ARG and "2^27" in text()
        assert call(pos=(C.c_int64 * nm)(10, 20, 19, 5, 6, 1, 1)) == ERR_ARG and "pos decreases inside a block (panel marker 2)" in text()
        assert call(pos=(C.c_int64 * nm)(10, 20, 30, 5, 6, 1, 0)) == ERR_ARG and "panel marker 6" in text()
        assert call(chrom=None) == ERR_ARG and "panel marker 3" in text()              # one block: the chromosome edges now count
        # what passes the rule stops at the missing context
        assert call() == ERR_ARG and "no context" in text()
        assert call(pairs=plist, npairs=3) == ERR_ARG and "no context" in text()       # a duplicate in the list is allowed
        assert call(dims=(C.c_long * 2)(16384, nm)) == ERR_ARG and "no context" in text()
        assert call(chrom=None, pos=None, seg=None, cap=0) == ERR_ARG and "no context" in text()
        assert call(prm=ref(params(mode=2, min_snp=1, merge_min=0, min_len=1 << 40, max_gap=1 << 40))) == ERR_ARG and "no context" in text()

    # the .bed entry point's own
    fn = L.eagle_bed_ibd
    good = (str(tmp_path / "p.bed").encode(), dims, None, None, 0, None, None, ref(params()), 8.0, tab, seg, 8, C.byref(total))
    names = ("path", "dims", "include", "pairs", "npairs", "chrom", "pos", "prm", "mem", "tab", "seg", "cap", "total")

    def call(**kw):
        return fn(None, *[kw.get(k, v) for k, v in zip(names, good)])
    assert call(dims=(C.c_long * 2)(1 << 30, nm)) == ERR_ARG and "2^30" in text()
    assert call(include=(C.c_uint8 * nm)()) == ERR_ARG and "no marker" in text()
    inc = (C.c_uint8 * nm)(1, 0, 1, 1, 0, 0, 0)
    assert call(include=inc, pos=(C.c_int64 * 3)(3, 2, 1)) == ERR_ARG and "panel marker 1" in text()        # pos is by PANEL marker
    assert call(include=inc, pos=(C.c_int64 * 3)(3, 2, 1), chrom=(C.c_int32 * 3)(1, 2, 3)) == ERR_ARG and "no context" in text()


def test_python_wrappers_refuse_before_the_library(tmp_path):
    from eagleeverything_amd import rcpp_api
    M, bed = str(tmp_path / "M.ascii"), str(tmp_path / "a.bed")
    for kw in (dict(chrom=[1, 1, 2]), dict(chrom=[1, 1.5, 2, 2, 2, 2]), dict(pos=[1, 2, 3]), dict(pos=[1, 2, 3, 4, 5, 6.5]),
               dict(pos=[1, 2, 3, 2, 5, 6]), dict(chrom=[1, 1, 1, 2, 2, 2], pos=[1, 2, 3, 1, 2, 1]), dict(mode=0), dict(mode=3), dict(mode="ibs3"),
               dict(mode=1.5), dict(min_snp=0), dict(min_len=-1), dict(max_gap=-1), dict(merge_min=-1), dict(merge_min=2.5), dict(window=50),
               dict(seg_cap=-1), dict(pairs=[[0, 0]]), dict(pairs=[[1, 0]]), dict(pairs=[[0, 4]]), dict(pairs=[[-1, 2]]), dict(pairs=[]),
               dict(pairs=[0, 1]), dict(pairs=[[0, 1.5]])):
        with pytest.raises(ValueError):
            rcpp_api.ibd(M, (4, 6), **kw)
        with pytest.raises(ValueError):
            rcpp_api.bed_ibd(bed, (4, 6), **kw)
    with pytest.raises(ValueError):
        rcpp_api.ibd(M, (1, 6))
    with pytest.raises(ValueError):
        rcpp_api.ibd(M, (16385, 6))
    with pytest.raises(ValueError):
        rcpp_api.bed_ibd(bed, (4, 6), include=[1, 0, 1])
    with pytest.raises(ValueError):
        rcpp_api.bed_ibd(bed, (4, 6), include=[1, 0, 1, 0, 1, 0], chrom=np.zeros(6))                  # chrom is by PANEL marker
    pr = rcpp_api.ibd_pairs("t", [[0, 1], [0, 1], [2, 3]], 4)
    assert pr.dtype == np.int32 and pr.flags["C_CONTIGUOUS"] and pr.tolist() == [[0, 1], [0, 1], [2, 3]]
    assert rcpp_api.ibd_pairs("t", None, 4) is None


def test_ibd_host_pieces_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ibd_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_ibd_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ibd host checks passed" in r.stdout
