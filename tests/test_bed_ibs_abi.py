"""CPU: the C ABI of the pairwise-complete counts without a device -- eagle_bed_sample_ibs and eagle_knn_rows_dist are declared,
exported and bound, the header states the definitions, and every argument error is decided before a context is needed (ctx == NULL:
the text comes through eagle_open_error).  No device work."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
NAMES = ("eagle_bed_sample_ibs", "eagle_knn_rows_dist")


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    assert len(_lib.SIGNATURES["eagle_bed_sample_ibs"][1]) == 11 and len(_lib.SIGNATURES["eagle_knn_rows_dist"][1]) == 5
    assert len(_lib.SIGNATURES["eagle_knn_rows"][1]) == 6          # the old entry keeps its signature
    for py in ("bed_sample_ibs", "knn_rows_dist"):
        assert callable(getattr(rcpp_api, py))


def test_header_states_the_definitions():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b'''ii."):txt.index("1b''''.")]         # the new section lies between kNN imputation and the GRM
    for phrase in ("g = -1, 0, 0, +1", "u = |g|", "h = [code == 2]", "c = [code != 1]", "D = g g^T", "N = c c^T",
                   "ibs0_ij = (Q_ij - D_ij) / 2", "hetsum_ij = H_ij + N_ij - Q_ij", "(double)(hethet_ij - 2 ibs0_ij) / (double)hetsum_ij",
                   "d_ij = 4 ibs0_ij + hetsum_ij - 2 hethet_ij", "(uint32)((int64)d_ij Linc / N_ij)", "0xFFFFFFFE", "L < 2^29",
                   "whatever bits they hold", "decided before the context is used"):
        assert phrase in sec, phrase
    assert txt.index("1b'''i.") < txt.index("1b'''ii.")


def test_interface_is_public():
    from eagleeverything_amd import r_api, rcpp_api
    for name in ("bed_ibs_host", "king_from_pair_counts", "knn_rows_host", "Relatedness", "ImputeBed"):
        assert callable(getattr(r_api, name))
    p = inspect.signature(rcpp_api.bed_sample_ibs).parameters
    assert list(p) == ["bed_path", "dims", "include", "min_overlap", "max_memory_in_Gbytes", "device"]
    assert (p["include"].default, p["min_overlap"].default, p["max_memory_in_Gbytes"].default, p["device"].default) == (None, 1, 8.0, 0)
    assert list(inspect.signature(rcpp_api.knn_rows_dist).parameters) == ["dist", "K", "device"]
    p = inspect.signature(r_api.Relatedness).parameters
    assert (p["bed"].default, p["include"].default, p["min_overlap"].default, p["threshold"].default) == (None, None, 1, 0.0884)
    p = inspect.signature(r_api.ImputeBed).parameters
    assert (p["pairwise"].default, p["min_overlap"].default, p["k"].default, p["K"].default) == (False, 1, 10, 64)
    p = inspect.signature(r_api.bed_ibs_host).parameters
    assert list(p) == ["codes", "include", "min_overlap"] and (p["include"].default, p["min_overlap"].default) == (None, 1)


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()
    n, nm = 5, 7
    fn = L.eagle_bed_sample_ibs
    m = [(C.c_int32 * (n * n))() for _ in range(4)]
    dist = (C.c_uint32 * (n * n))()
    inc = (C.c_uint8 * nm)(*([1] * nm))
    good = (str(tmp_path / "in.bed").encode(), (C.c_long * 2)(n, nm), inc, 1, 8.0, m[0], m[1], m[2], m[3], dist)
    names = ("bed_path", "dims", "include", "min_overlap", "mem", "ncalled", "ibs0", "hethet", "hetsum", "dist")

    def call(**kw):
        return fn(None, *[kw[nm_] if nm_ in kw else v for nm_, v in zip(names, good)])
    for arg in ("bed_path", "dims", "ncalled", "ibs0", "hethet", "hetsum"):
        assert call(**{arg: None}) == ERR_ARG and "bed_sample_ibs" in text() and "NULL" in text(), arg
    assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(n, 0)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(-1, nm)) == ERR_ARG
    assert call(dims=(C.c_long * 2)(n, 1 << 29)) == ERR_ARG and "2^29" in text()
    assert call(dims=(C.c_long * 2)(n, (1 << 29) - 1)) == ERR_ARG and "no context" in text()
    assert call(min_overlap=0) == ERR_ARG and "min_overlap" in text()
    assert call(min_overlap=-5) == ERR_ARG and "min_overlap" in text()
    assert call() == ERR_ARG and "no context" in text()
    assert call(include=None) == ERR_ARG and "no context" in text()          # include and dist_out may be NULL
    assert call(dist=None) == ERR_ARG and "no context" in text()

    fn = L.eagle_knn_rows_dist
    nbr_out = (C.c_int32 * (n * 256))()
    assert fn(None, None, n, 3, nbr_out) == ERR_ARG and "knn_rows_dist" in text() and "NULL" in text()
    assert fn(None, dist, n, 3, None) == ERR_ARG and "NULL" in text()
    assert fn(None, dist, 0, 3, nbr_out) == ERR_ARG and "positive" in text()
    assert fn(None, dist, -1, 3, nbr_out) == ERR_ARG
    assert fn(None, dist, 32769, 3, nbr_out) == ERR_ARG and "EAGLE_KNN_MAX_N" in text()
    assert fn(None, dist, n, 0, nbr_out) == ERR_ARG and "K outside" in text()
    assert fn(None, dist, n, 257, nbr_out) == ERR_ARG and "K outside" in text()
    assert fn(None, dist, n, 256, nbr_out) == ERR_ARG and "no context" in text()


def test_python_wrappers_refuse_before_the_library(tmp_path):
    from eagleeverything_amd import rcpp_api
    with pytest.raises(ValueError):
        rcpp_api.bed_sample_ibs(str(tmp_path / "a.bed"), (4, 6), include=np.ones(5, dtype=bool))
    with pytest.raises(ValueError):
        rcpp_api.knn_rows_dist(np.zeros((3, 4), dtype=np.uint32), 2)
    with pytest.raises(ValueError):
        rcpp_api.knn_rows_dist(np.zeros((3, 3)) + 0.5, 2)
