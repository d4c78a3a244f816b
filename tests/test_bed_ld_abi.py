"""CPU: the C ABI of pairwise-complete LD from a .bed file without a device -- eagle_bed_ld_window and eagle_bed_ld_partners are declared,
exported and bound with the header's argument lists, the header states the definition and the window rule, and every argument error is
decided before a context is needed (ctx == NULL: the text comes through eagle_open_error).  No device work."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
NAMES = ("eagle_bed_ld_window", "eagle_bed_ld_partners")
CTYPE_OF = {"eagle_ctx*": C.c_void_p, "const char*": C.c_char_p, "const long*": "lp", "const uint8_t*": C.c_void_p, "long": C.c_long,
            "int": C.c_int, "double": C.c_double, "uint64_t*": C.POINTER(C.c_uint64), "long*": "lp", "const int32_t*": C.POINTER(C.c_int32),
            "int32_t*": C.POINTER(C.c_int32), "double*": "dp"}


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def declared_args(name):
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name + " is not declared in include/eagle_hip.h"
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        arr = a.endswith("]")
        ty, arg = re.sub(r"\[\d*\]$", "", a).rsplit(" ", 1)           # "const long dims[2]" -> ("const long", "dims"): a pointer
        out.append((ty.replace(" *", "*") + ("*" if arr else ""), arg))
    return out


def test_declarations_match_the_bindings():
    from eagleeverything_amd import _lib, rcpp_api
    from eagleeverything_amd._lib import c_dp, c_lp
    L = _lib.load()
    want = {"eagle_bed_ld_window": ["ctx", "bed_path", "dims", "include", "window", "r2", "min_overlap", "max_memory_in_Gbytes", "mask_out",
                                    "npairs_out"],
            "eagle_bed_ld_partners": ["ctx", "bed_path", "dims", "include", "window", "l", "min_r2", "min_overlap", "chrom",
                                      "max_memory_in_Gbytes", "partners_out", "r2_out"]}
    for name in NAMES:
        args = declared_args(name)
        assert [a for _, a in args] == want[name]
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        res, bound = _lib.SIGNATURES[name]
        assert res is C.c_int and len(bound) == len(args)
        for (ty, arg), b in zip(args, bound):
            c = CTYPE_OF[ty]
            c = c_lp if c == "lp" else (c_dp if c == "dp" else c)
            assert b is c, (name, arg, ty, b)
    for py in ("bed_ld_window", "bed_ld_partners"):
        assert callable(getattr(rcpp_api, py))


def test_header_states_the_definition_and_the_window_rule():
    txt = " ".join(header().replace("*", " ").split())
    assert txt.index("1b'''iii.") < txt.index("1b'''iv.") < txt.index("1b''''.")
    sec = txt[txt.index("1b'''iv."):txt.index("1b''''.")]
    for phrase in ("N = sum c_i c_j", "D = sum x_i x_j", "Si = sum x_i c_j", "Sj = sum c_i x_j", "Qi = sum u_i c_j", "Qj = sum c_i u_j",
                   "cov = N D - Si Sj", "vi = N Qi - Si^2", "vj = N Qj - Sj^2", "COMPARABLE iff N >= min_overlap, vi > 0 and vj > 0",
                   "(double)cov (double)cov > t ((double)vi (double)vj)", "r2 = fl( fl(dc dc) / fl(dvi dvj) )", "its r2 entry is -1.0",
                   "bit for bit those of eagle_ld_window and eagle_ld_partners", "n <= 0x3fffffff", "belong to nobody",
                   "S = max(1, floor(min(64 MiB, max_memory_in_Gbytes 1e9 / 4) / rb))", "Wmax = max(1024, floor(2^27 / ld))",
                   "need = window + 1 for eagle_bed_ld_window and 2 window + 1 for eagle_bed_ld_partners", "starts at hi - window",
                   "hi - 2 window", "does not depend on the window size", "decided before the context is used"):
        assert phrase in sec, phrase


def test_interface_is_public_and_defaults_are_todays():
    from eagleeverything_amd import r_api, rcpp_api
    assert list(inspect.signature(rcpp_api.bed_ld_window).parameters) == ["bed_path", "dims", "window", "r2", "include", "min_overlap", "availmemGb",
                                                                          "device", "return_pairs"]
    assert list(inspect.signature(rcpp_api.bed_ld_partners).parameters) == ["bed_path", "dims", "window", "l", "min_r2", "include", "min_overlap",
                                                                            "chrom", "availmemGb", "device", "return_r2"]
    p = inspect.signature(rcpp_api.bed_ld_window).parameters
    assert (p["include"].default, p["min_overlap"].default, p["availmemGb"].default, p["return_pairs"].default) == (None, 1, 8.0, False)
    assert list(inspect.signature(r_api.bed_ld_host).parameters) == ["codes", "window", "include", "min_overlap"]
    assert list(inspect.signature(r_api.bed_ld_mask_host).parameters) == ["codes", "window", "r2", "include", "min_overlap"]
    assert list(inspect.signature(r_api.bed_ld_partners_host).parameters) == ["codes", "window", "l", "min_r2", "include", "min_overlap", "chrom"]
    p = inspect.signature(r_api.LDPrune).parameters
    assert (p["bed"].default, p["min_overlap"].default) == (None, None)
    p = inspect.signature(r_api.ImputeBed).parameters
    assert (p["ld_from"].default, p["ld_min_overlap"].default) == ("panel", None)
    assert inspect.signature(r_api.ReadMarker).parameters["impute_ld_from"].default == "panel"
    with pytest.raises(ValueError):
        r_api.ImputeBed("a", {"dim_of_ascii_M": [2, 2]}, "b", local=2, ld_from="file")


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()

    n, nm = 5, 7
    dims = (C.c_long * 2)(n, nm)
    bed = str(tmp_path / "in.bed").encode()
    inc = (C.c_uint8 * nm)(1, 0, 1, 1, 0, 0, 1)
    none = (C.c_uint8 * nm)()
    mask = (C.c_uint64 * (nm * 4))()
    pairs = C.c_long(0)
    fn = L.eagle_bed_ld_window
    good = (bed, dims, inc, 50, 0.2, 1, 8.0, mask, C.byref(pairs))

    def call(**kw):
        names = ("path", "dims", "include", "window", "r2", "min_overlap", "mem", "mask", "pairs")
        return fn(None, *[kw.get(nm_, v) for nm_, v in zip(names, good)])
    assert call(path=None) == ERR_ARG and "bed_ld_window" in text() and "NULL" in text()
    assert call(dims=None) == ERR_ARG
    assert call(mask=None) == ERR_ARG
    assert call(pairs=None) == ERR_ARG
    assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(n, -1)) == ERR_ARG
    assert call(dims=(C.c_long * 2)(1 << 30, nm)) == ERR_ARG and "2^30" in text()
    assert call(window=0) == ERR_ARG and "window" in text()
    assert call(window=257) == ERR_ARG
    assert call(r2=-0.01) == ERR_ARG and "r2" in text()
    assert call(r2=1.01) == ERR_ARG
    assert call(r2=float("nan")) == ERR_ARG
    assert call(min_overlap=0) == ERR_ARG and "min_overlap" in text()
    assert call(min_overlap=-3) == ERR_ARG
    assert call(include=none) == ERR_ARG and "selects no marker" in text()
    assert call() == ERR_ARG and "no context" in text()
    assert call(include=None) == ERR_ARG and "no context" in text()                      # include may be NULL
    assert call(window=256, r2=1.0, min_overlap=1 << 30) == ERR_ARG and "no context" in text()   # the limits themselves pass
    assert call(window=1, r2=0.0, dims=(C.c_long * 2)((1 << 30) - 1, nm)) == ERR_ARG and "no context" in text()

    fn = L.eagle_bed_ld_partners
    part = (C.c_int32 * (nm * 32))()
    r2 = (C.c_double * (nm * 32))()
    chrom = (C.c_int32 * nm)()
    good = (bed, dims, inc, 50, 4, 0.0, 1, chrom, 8.0, part, r2)

    def call(**kw):
        names = ("path", "dims", "include", "window", "l", "min_r2", "min_overlap", "chrom", "mem", "part", "r2")
        return fn(None, *[kw.get(nm_, v) for nm_, v in zip(names, good)])
    assert call(path=None) == ERR_ARG and "bed_ld_partners" in text() and "NULL" in text()
    assert call(dims=None) == ERR_ARG
    assert call(part=None) == ERR_ARG
    assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(n, 0)) == ERR_ARG
    assert call(dims=(C.c_long * 2)(1 << 30, nm)) == ERR_ARG and "2^30" in text()
    assert call(window=0) == ERR_ARG and "window" in text()
    assert call(window=257) == ERR_ARG
    assert call(l=0) == ERR_ARG and "l outside" in text()
    assert call(l=33) == ERR_ARG
    assert call(min_r2=-0.01) == ERR_ARG and "min_r2" in text()
    assert call(min_r2=1.01) == ERR_ARG
    assert call(min_r2=float("nan")) == ERR_ARG
    assert call(min_overlap=0) == ERR_ARG and "min_overlap" in text()
    assert call(include=none) == ERR_ARG and "selects no marker" in text()
    assert call(include=None, dims=(C.c_long * 2)(n, 1 << 31)) == ERR_ARG and "2^31" in text()   # Linc = L without include
    assert call() == ERR_ARG and "no context" in text()
    assert call(include=None, chrom=None, r2=None) == ERR_ARG and "no context" in text()         # include, chrom and r2_out may be NULL
    assert call(window=256, l=32, min_r2=1.0) == ERR_ARG and "no context" in text()


def test_python_wrappers_refuse_before_the_library(tmp_path):
    from eagleeverything_amd import rcpp_api
    bed = str(tmp_path / "a.bed")
    with pytest.raises(ValueError):
        rcpp_api.bed_ld_window(bed, (4, 6), include=[1, 0, 1])                                   # one per marker of the file
    with pytest.raises(ValueError):
        rcpp_api.bed_ld_partners(bed, (4, 6), include=np.ones(5))
    with pytest.raises(ValueError):
        rcpp_api.bed_ld_partners(bed, (4, 6), include=[1, 0, 1, 1, 0, 1], chrom=[1] * 6)         # chrom is per PANEL marker
    with pytest.raises(ValueError):
        rcpp_api.bed_ld_partners(bed, (4, 3), chrom=[1, 1.5, 2])
    with pytest.raises(rcpp_api.EagleError):
        rcpp_api.bed_ld_window(bed, (4, 6), include=np.zeros(6))                                 # selects no marker: the library's text
