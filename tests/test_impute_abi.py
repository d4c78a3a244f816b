"""CPU: the C ABI of kNN imputation without a device -- eagle_knn_rows and eagle_bed_impute_knn are declared, exported and bound, the
header states the definitions and the limits, and every argument error is decided before a context is needed (ctx == NULL: the
text comes through eagle_open_error).  No device work."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
I32P = C.POINTER(C.c_int32)
NAMES = ("eagle_knn_rows", "eagle_bed_impute_knn")


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_impute_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    assert len(_lib.SIGNATURES["eagle_knn_rows"][1]) == 6 and len(_lib.SIGNATURES["eagle_bed_impute_knn"][1]) == 10
    for py in ("knn_rows", "bed_impute_knn"):
        assert callable(getattr(rcpp_api, py))
    for macro, value in (("EAGLE_KNN_MAX_K", "256"), ("EAGLE_KNN_MAX_N", "32768L"), ("EAGLE_IMPUTE_MAX_N", "245760L")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, value), txt), macro


def test_header_states_the_definitions():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b'''i."):txt.index("1b''''.")]          # the new section lies between sample QC and the GRM
    for phrase in ("d_ij = 4 ibs0_ij + h_i + h_j - 2 hethet_ij", "(uint64)(uint32)d_ij << 32 | j", "K_eff = min(K, n - 1)",
                   "(2 s + c) / (2 c)", "c = n0 + n1 + n2, s = n1 + 2 n2", "written as 00", "does not depend on the order",
                   "decided before the context is used"):
        assert phrase in sec, phrase
    assert txt.index("1b'''.") < txt.index("1b'''i.")


def test_impute_interface_is_public():
    from eagleeverything_amd import r_api
    for name in ("knn_distance", "knn_rows_host", "impute_knn_host", "ImputeBed", "read_bed_codes", "pack_bed_codes"):
        assert callable(getattr(r_api, name))
    p = inspect.signature(r_api.ImputeBed).parameters
    assert list(p)[:3] == ["bed", "geno", "out_prefix"]
    assert (p["k"].default, p["K"].default, p["min_votes"].default, p["availmemGb"].default) == (10, 64, 1, 8)
    assert inspect.signature(r_api.ReadMarker).parameters["impute"].default is None


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()
    n = 5
    m = (C.c_int32 * (n * n))()
    nbr_out = (C.c_int32 * (n * 256))()
    fn = L.eagle_knn_rows
    assert fn(None, None, m, n, 3, nbr_out) == ERR_ARG and "knn_rows" in text() and "NULL" in text()
    assert fn(None, m, None, n, 3, nbr_out) == ERR_ARG
    assert fn(None, m, m, n, 3, None) == ERR_ARG
    assert fn(None, m, m, 0, 3, nbr_out) == ERR_ARG and "positive" in text()
    assert fn(None, m, m, -1, 3, nbr_out) == ERR_ARG
    assert fn(None, m, m, 32769, 3, nbr_out) == ERR_ARG and "EAGLE_KNN_MAX_N" in text()
    assert fn(None, m, m, n, 0, nbr_out) == ERR_ARG and "K outside" in text()
    assert fn(None, m, m, n, 257, nbr_out) == ERR_ARG
    assert fn(None, m, m, n, 256, nbr_out) == ERR_ARG and "no context" in text()

    fn = L.eagle_bed_impute_knn
    K = 3
    dims = (C.c_long * 2)(n, 7)
    nbr = (C.c_int32 * (n * K))(*([1, 2, -1] * n))
    counts = (C.c_int32 * 14)()
    src, dst = str(tmp_path / "in.bed").encode(), str(tmp_path / "out.bed").encode()
    good = (src, dims, nbr, K, 2, 1, dst, 8.0, counts)

    def call(**kw):
        names = ("bed_path", "dims", "nbr", "K", "k", "min_votes", "out", "mem", "counts")
        return fn(None, *[kw.get(nm, v) for nm, v in zip(names, good)])
    assert call(bed_path=None) == ERR_ARG and "bed_impute_knn" in text() and "NULL" in text()
    assert call(dims=None) == ERR_ARG
    assert call(nbr=None) == ERR_ARG
    assert call(out=None) == ERR_ARG
    assert call(dims=(C.c_long * 2)(0, 7)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(n, -2)) == ERR_ARG
    assert call(dims=(C.c_long * 2)(245761, 7)) == ERR_ARG and "EAGLE_IMPUTE_MAX_N" in text()
    assert call(K=0) == ERR_ARG and "K outside" in text()
    assert call(K=257) == ERR_ARG
    assert call(k=0) == ERR_ARG and "k outside" in text()
    assert call(k=K + 1) == ERR_ARG
    assert call(min_votes=0) == ERR_ARG and "min_votes" in text()
    assert call(out=src) == ERR_ARG and "differ" in text()
    for bad in (-2, n, 1 << 30):
        v = [1, 2, -1] * n
        v[7] = bad
        assert call(nbr=(C.c_int32 * (n * K))(*v)) == ERR_ARG and "neighbour" in text()
    assert call() == ERR_ARG and "no context" in text()
    assert call(counts=None) == ERR_ARG and "no context" in text()          # counts_out may be NULL
    assert not os.path.exists(dst)


def test_python_wrappers_refuse_before_the_library(tmp_path):
    from eagleeverything_amd import rcpp_api
    with pytest.raises(ValueError):
        rcpp_api.knn_rows(np.zeros((3, 3)), np.zeros((3, 4)), 2)
    with pytest.raises(ValueError):
        rcpp_api.knn_rows(np.zeros((3, 3)) + 0.5, np.zeros((3, 3)), 2)
    with pytest.raises(ValueError):
        rcpp_api.bed_impute_knn(str(tmp_path / "a.bed"), (4, 2), np.zeros((3, 2), dtype=np.int32), 1, 1, str(tmp_path / "b.bed"))


def test_regime_thresholds_of_the_kernels_are_where_the_gpu_cases_expect_them():
    """tests/test_gpu_regimes.py runs k_bed_impute on both sides of these thresholds and the two kNN kernels at their LDS maximum; a
    change here must move its cases (tests/regimes_truth.py restates the arithmetic)."""
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_impute.hip")).read())
    flat = " ".join(src.split())
    assert "#define IMP_STAGE_BYTES (EAGLE_IMPUTE_MAX_N / 4)" in flat and "#define IMP_MAX_ROWS 256" in flat
    assert "std::max(1L, std::min(std::min((long)IMP_STAGE_BYTES / rb, (long)IMP_MAX_ROWS), std::max(1L, 16384L / rb)))" in flat
    assert "__shared__ uint8_t stage[IMP_STAGE_BYTES];" in flat and "__shared__ int cnt[IMP_MAX_ROWS][2];" in flat
    # the two thread layouts: all three uses of the threshold, and the 256 threads they are written for
    assert flat.count("rb >= 256") == 3 and "const int rpp = rb >= 256 ? 1 : (int)(256 / rb);" in flat
    assert "const int sub = rb >= 256 ? 0 : (int)(tid / rb);" in flat and "for (long b = rb >= 256 ? tid : tid - sub * rb; b < rb; b += 256)" in flat
    assert "hipLaunchKernelGGL(k_bed_impute, dim3((unsigned)blocks), dim3(256), 0," in flat
    # 4 n bytes of dynamic LDS, allowed up to 4 EAGLE_KNN_MAX_N
    assert flat.count("hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (int)EAGLE_KNN_MAX_N") == 2
    assert flat.count("dim3((unsigned)n), dim3(256), (size_t)(4 * n)") == 2 and "for (int j = tid; j < n; j += 256)" in flat
