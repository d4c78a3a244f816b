"""CPU: the C ABI of LD-kNNi without a device -- eagle_ld_partners and eagle_bed_impute_ldknn are declared, exported and bound, the
header states the definitions and the three limits, and every argument error is decided before a context is needed (ctx == NULL: the
text comes through eagle_open_error).  No device work."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
NAMES = ("eagle_ld_partners", "eagle_bed_impute_ldknn")


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_ldknn_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    assert len(_lib.SIGNATURES["eagle_ld_partners"][1]) == 10 and len(_lib.SIGNATURES["eagle_bed_impute_ldknn"][1]) == 11
    for py in ("ld_partners", "bed_impute_ldknn"):
        assert callable(getattr(rcpp_api, py))
    for macro, value in (("EAGLE_LDKNN_MAX_PARTNERS", "32"), ("EAGLE_LDKNN_MAX_K", "64"), ("EAGLE_LDKNN_MAX_N", "12288L")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, value), txt), macro
    assert (rcpp_api.LDKNN_MAX_PARTNERS, rcpp_api.LDKNN_MAX_K, rcpp_api.LDKNN_MAX_N) == (32, 64, 12288)
    assert rcpp_api.LDKNN_MAX_N >= 8192 and 12.5 * rcpp_api.LDKNN_MAX_N + 1024 <= 160 * 1024      # the LDS of a compute unit


def test_header_states_the_definitions():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b'''iii."):txt.index("1b''''.")]
    for phrase in ("r2_ij = fl( fl((double)c (double)c) / fl((double)v_i (double)v_j) )", "1 <= |j - i| <= window", "decreasing r2",
                   "smaller |j - i|", "dist_ij = (d_ij 4096) / ov_ij", "(uint64)dist_ij << 32 | j", "(2 s + c) / (2 c)", "written as 00",
                   "does not depend on the order", "decided before the context is used", "more than 256 rows from its marker"):
        assert phrase in sec, phrase
    assert txt.index("1b'''ii.") < txt.index("1b'''iii.")


def test_ldknn_interface_is_public():
    from eagleeverything_amd import r_api, rcpp_api
    for name in ("ld_partners_host", "impute_ldknn_host", "ImputeBed"):
        assert callable(getattr(r_api, name))
    p = inspect.signature(r_api.ImputeBed).parameters
    assert (p["local"].default, p["window"].default, p["min_r2"].default, p["local_min_overlap"].default, p["map"].default) == (None, 50, 0.0, 4, None)
    assert inspect.signature(r_api.ReadMarker).parameters["impute_local"].default is None
    p = inspect.signature(rcpp_api.ld_partners).parameters
    assert (p["window"].default, p["l"].default, p["min_r2"].default, p["chrom"].default, p["return_r2"].default) == (50, 16, 0.0, None, False)
    assert list(inspect.signature(rcpp_api.bed_impute_ldknn).parameters)[:7] == ["bed_path", "dims", "partners", "k", "min_votes", "min_overlap",
                                                                                  "out_bed_path"]
    assert list(inspect.signature(r_api.ld_partners_host).parameters) == ["Mt8", "window", "l", "min_r2", "chrom"]
    assert list(inspect.signature(r_api.impute_ldknn_host).parameters) == ["codes", "partners", "k", "min_votes", "min_overlap"]


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()

    fn = L.eagle_ld_partners
    nm, l = 7, 4
    dims = (C.c_long * 2)(5, nm)
    part = (C.c_int32 * (nm * 32))()
    r2 = (C.c_double * (nm * 32))()
    chrom = (C.c_int32 * nm)()
    good = (str(tmp_path / "Mt.ascii").encode(), dims, 50, l, 0.0, chrom, 8.0, part, r2)

    def call(**kw):
        names = ("path", "dims", "window", "l", "min_r2", "chrom", "mem", "part", "r2")
        return fn(None, *[kw.get(nm_, v) for nm_, v in zip(names, good)])
    assert call(path=None) == ERR_ARG and "ld_partners" in text() and "NULL" in text()
    assert call(dims=None) == ERR_ARG
    assert call(part=None) == ERR_ARG
    assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(5, -1)) == ERR_ARG
    assert call(dims=(C.c_long * 2)(5, 1 << 31)) == ERR_ARG and "2^31" in text()
    assert call(window=0) == ERR_ARG and "window" in text()
    assert call(window=257) == ERR_ARG
    assert call(l=0) == ERR_ARG and "l outside" in text()
    assert call(l=33) == ERR_ARG
    assert call(min_r2=-0.01) == ERR_ARG and "min_r2" in text()
    assert call(min_r2=1.01) == ERR_ARG
    assert call(min_r2=float("nan")) == ERR_ARG
    assert call() == ERR_ARG and "no context" in text()
    assert call(window=256, l=32, min_r2=1.0) == ERR_ARG and "no context" in text()      # the limits themselves pass
    assert call(chrom=None, r2=None) == ERR_ARG and "no context" in text()               # chrom and r2_out may be NULL

    fn = L.eagle_bed_impute_ldknn
    n, nm, l = 5, 300, 3
    dims = (C.c_long * 2)(n, nm)
    base = [-1] * (nm * l)
    base[0:3] = [1, 2, 256]                                                 # marker 0: 256 rows away is the limit
    base[3 * 299:3 * 299 + 2] = [43, 298]                                   # marker 299: again
    counts = (C.c_int32 * (2 * nm))()
    src, dst = str(tmp_path / "in.bed").encode(), str(tmp_path / "out.bed").encode()
    good = (src, dims, (C.c_int32 * (nm * l))(*base), l, 5, 1, 2, dst, 8.0, counts)

    def call(**kw):
        names = ("bed_path", "dims", "partners", "l", "k", "min_votes", "min_overlap", "out", "mem", "counts")
        return fn(None, *[kw.get(nm_, v) for nm_, v in zip(names, good)])
    assert call(bed_path=None) == ERR_ARG and "bed_impute_ldknn" in text() and "NULL" in text()
    assert call(dims=None) == ERR_ARG
    assert call(partners=None) == ERR_ARG
    assert call(out=None) == ERR_ARG
    assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(n, -2)) == ERR_ARG
    assert call(dims=(C.c_long * 2)(12289, nm)) == ERR_ARG and "EAGLE_LDKNN_MAX_N" in text()
    assert call(l=0) == ERR_ARG and "l outside" in text()
    assert call(l=33) == ERR_ARG
    assert call(k=0) == ERR_ARG and "k outside" in text()
    assert call(k=65) == ERR_ARG
    assert call(min_votes=0) == ERR_ARG and "min_votes" in text()
    assert call(min_overlap=0) == ERR_ARG and "min_overlap" in text()
    assert call(min_overlap=33) == ERR_ARG
    assert call(out=src) == ERR_ARG and "differ" in text()
    for bad in (-2, nm, 1 << 30):
        v = list(base)
        v[7] = bad
        assert call(partners=(C.c_int32 * (nm * l))(*v)) == ERR_ARG and "outside [-1, L)" in text()
    for m, bad in ((0, 257), (299, 42), (20, 277)):
        v = list(base)
        v[3 * m + 1] = bad
        assert call(partners=(C.c_int32 * (nm * l))(*v)) == ERR_ARG and "256 rows" in text()
    assert call() == ERR_ARG and "no context" in text()
    assert call(k=64, min_overlap=32, min_votes=1000) == ERR_ARG and "no context" in text()   # min_votes has no upper limit
    assert call(counts=None) == ERR_ARG and "no context" in text()                            # counts_out may be NULL
    assert call(dims=(C.c_long * 2)(12288, nm)) == ERR_ARG and "no context" in text()
    assert not os.path.exists(dst)


def test_python_wrappers_refuse_before_the_library(tmp_path):
    from eagleeverything_amd import rcpp_api
    with pytest.raises(ValueError):
        rcpp_api.ld_partners(str(tmp_path / "Mt.ascii"), (4, 6), chrom=[1, 1, 2])                      # one per marker
    with pytest.raises(ValueError):
        rcpp_api.ld_partners(str(tmp_path / "Mt.ascii"), (4, 3), chrom=[1, 1.5, 2])
    with pytest.raises(ValueError):
        rcpp_api.bed_impute_ldknn(str(tmp_path / "a.bed"), (4, 2), np.zeros((3, 2), dtype=np.int32), 1, 1, 1, str(tmp_path / "b.bed"))
    with pytest.raises(ValueError):
        rcpp_api.bed_impute_ldknn(str(tmp_path / "a.bed"), (4, 2), np.zeros((2, 2)) + 0.5, 1, 1, 1, str(tmp_path / "b.bed"))


def test_regime_thresholds_of_the_kernel_are_where_the_gpu_cases_expect_them():
    """tests/test_gpu_regimes.py runs k_bed_impute_ldknn past one trip of its 512-thread column loops and at 150 KiB of LDS; a change
    here must move its cases (tests/regimes_truth.py restates the arithmetic)."""
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ldknn.hip")).read())
    flat = " ".join(src.split())
    assert "#define LDK_THREADS 512" in flat and "__launch_bounds__(LDK_THREADS)" in flat and "dim3(LDK_THREADS), ldk_lds_bytes(n)" in flat
    assert "return (size_t)(3 * ((n + 3) / 4 * 4) + 2 * ((bed_row_bytes(n) + 3) / 4)) * 4;" in flat
    assert "for (int b = tid; b < (int)rb; b += LDK_THREADS)" in flat and flat.count("for (long b = tid; b < rb; b += LDK_THREADS)") == 2
    assert "for (int b = tid; b < 4 * rbw; b += LDK_THREADS)" in flat
    assert "hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldk_lds_bytes(EAGLE_LDKNN_MAX_N)" in flat
    assert re.search(r"#define\s+EAGLE_LDKNN_MAX_N\s+12288L", open(os.path.join(ROOT, "include", "eagle_hip.h")).read())
