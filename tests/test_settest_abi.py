"""CPU: the C ABI of the set test without a device -- eagle_spectral_settest is declared, exported and bound with its argument count,
section 1d'' of the header states the rule, every argument error that needs no context is decided before one is needed (ctx == NULL:
the text comes through eagle_open_error), the Python wrapper refuses malformed input before the library is called, and the README
names the feature and its limits.  The errors that need the n and L of a prepared context (a marker index >= L, lambda, a non-finite
operand, n <= c + 1, no prepare, a multi-device context) are in tests/test_gpu_settest.py.  No device work."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_settest_symbol_declared_exported_and_bound():
    from eagleeverything_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    assert re.search(r"\bint\s+eagle_spectral_settest\s*\(\s*eagle_ctx\s*\*", txt), "eagle_spectral_settest is not declared in include/eagle_hip.h"
    assert re.search(r"#define\s+SETTEST_MAX_MARKERS\s+64\b", txt)
    assert hasattr(L, "eagle_spectral_settest"), "libeaglehip.so does not export eagle_spectral_settest"
    sig = _lib.SIGNATURES["eagle_spectral_settest"]
    assert sig[0] is C.c_int and len(sig[1]) == 15
    decl = re.search(r"int\s+eagle_spectral_settest\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
    assert len(decl.split(",")) == 15
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_settest.hip" in makefile and "eagle_settest.o" in makefile
    kern = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_settest.hip")).read()
    code = re.sub(r"//.*", "", kern)
    assert "k_settest_gram" in code and code.count("__builtin_amdgcn_mfma_f64_16x16x4f64") == 1    # one instruction form: A = d x, B = x
    assert "asm" not in code and "atomic" not in code.lower()


def test_header_states_the_rule():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1d''."):txt.index("#define SETTEST_MAX_MARKERS")]
    for phrase in ("burden test and SKAT", "EMMAX-SKAT / famSKAT", "r_api.settest_host", "k_settest_gram", "d_k = 1 / (varE + varG lambda_k)",
                   "1 <= m <= SETTEST_MAX_MARKERS = 64", "finite and >= 0", "set_ptr[nsets + 1]", "A marker may be in many sets",
                   "G = A^T diag(d) A", "A = [z_j1 .. z_jm | Xt | yt]", "v_mfma_f64_16x16x4_f64", "LMM_PIVOT_REL times its diagonal entry of G_xx",
                   "an argument error of the whole call", "B = G_xx^-1 [G_xz | G_xy]", "s = varG (G_zy - G_zx B_y)",
                   "Phi = varG^2 (G_zz - G_zx B_z)", "Phi_jj <= LMM_PIVOT_REL varG^2 (G_zz)_jj", "a monomorphic marker, a marker in the span of X",
                   "set to exactly 0", "n_degenerate", "Q = sum_j omega_j^2 s_j^2", "Ub = sum_j omega_j s_j", "Vb = omega^T Phi omega",
                   "c_r = tr(Aw^r) for r = 1 .. 4", "symmetric bit for bit: the mirror is a copy of the lower triangle",
                   "stat_out[7 o ..] = (Q, Ub, Vb, c_1, c_2, c_3, c_4)", "info_out[2 o ..] = (code, m - n_degenerate)", "2 nothing left",
                   "the seven statistics are NaN", "may each be NULL", "for any order of the sets, for a set listed twice and for a second call",
                   "WITHIN a set is not claimed", "bit equality with the host restatement is not claimed", "sets above 64 markers",
                   "SKAT-O's rho grid", "c outside [1, 14]", "nsets < 0", "set_ptr not non-decreasing from 0", "an empty set",
                   "a negative or non-finite weight", "a negative marker index", "a multi-device context", "no eagle_spectral_prepare",
                   "n <= c + 1", "a marker index >= L", "varE + varG lambda_k <= 0", "a non-finite entry of UtX or Uty",
                   "nsets == 0 returns EAGLE_OK"):
        assert phrase in sec, phrase
    assert txt.index("1d'.") < txt.index("1d''.") < txt.index(" 2. Device-resident entry points")


def test_readme_and_design_name_the_feature_and_its_limits():
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    for phrase in ("SetTest(", "eagle_spectral_settest", "64 markers", "SKAT-O", "Not claimed"):
        assert phrase in readme, phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_settest_gram" in design and "ScratchSize" in design
    assert os.path.exists(os.path.join(ROOT, "tools", "settest_timing.py"))


def test_settest_interface_is_public():
    import eagleeverything_amd
    from eagleeverything_amd import am, r_api, rcpp_api
    assert "SetTest" in eagleeverything_amd.__doc__
    p = inspect.signature(am.SetTest).parameters
    assert list(p)[:4] == ["trait", "X", "geno", "sets"]
    assert [(k, p[k].default) for k in list(p)[4:8]] == [("weights", "equal"), ("p_refine", 1e-3), ("backend", None), ("map", None)]
    assert list(inspect.signature(r_api.SetTest).parameters) == list(p)
    assert list(inspect.signature(r_api.settest_host).parameters) == ["lam", "UtX", "Uty", "Zrows", "varE", "varG", "sets", "omega"]
    p = inspect.signature(r_api.skat_pvalue).parameters
    assert [(k, p[k].default) for k in p] == [("Q", inspect.Parameter.empty), ("c", None), ("eig", None), ("method", "liu")]
    assert list(inspect.signature(r_api.sets_from_windows).parameters) == ["L_or_map", "size", "step", "kb"]
    assert list(inspect.signature(r_api.sets_from_table).parameters) == ["map", "regions"]
    assert rcpp_api.SETTEST_MAX_MARKERS == r_api.SETTEST_MAX_MARKERS == 64
    assert list(inspect.signature(rcpp_api.spectral_settest).parameters)[:7] == ["lam", "UtX", "Uty", "varE", "varG", "sets", "omega"]


def test_python_wrapper_refuses_before_the_library(monkeypatch):
    from eagleeverything_amd import _lib, rcpp_api
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    n = 8
    lam, UtX, Uty = np.linspace(1.0, 2.0, n), np.ones((n, 2)), np.arange(float(n))
    nan_lam = lam.copy()
    nan_lam[3] = np.nan
    bad = [dict(UtX=np.ones((n - 1, 2))), dict(UtX=np.ones((n, 15))), dict(UtX=np.ones((n, 0))), dict(Uty=np.ones(n + 1)), dict(lam=nan_lam),
           dict(UtX=np.full((n, 2), np.inf)), dict(varE=float("nan")), dict(varG=float("inf")), dict(sets=[[0, 1], []]),
           dict(sets=[list(range(65))]), dict(sets=[[0, -1]]), dict(sets=[[[0, 1], [2, 3]]]), dict(omega=[[1.0, -1.0]]),
           dict(omega=[[1.0, float("nan")]]), dict(omega=[[1.0]]), dict(omega=np.ones(3))]
    for kw in bad:
        args = dict(lam=lam, UtX=UtX, Uty=Uty, varE=1.0, varG=1.0, sets=[[0, 1]], omega=None)
        args.update(kw)
        with pytest.raises(ValueError):
            rcpp_api.spectral_settest(**args)
    ptr, idx, w = rcpp_api.settest_csr([[3, 1], [2]], [[0.5, 2.0], [1.0]])
    assert list(ptr) == [0, 2, 3] and list(idx) == [3, 1, 2] and list(w) == [0.5, 2.0, 1.0] and ptr.dtype == idx.dtype == np.int64
    assert list(rcpp_api.settest_csr([[3, 1], [2]])[2]) == [1.0, 1.0, 1.0]


def test_c_argument_errors_need_no_context():
    from eagleeverything_amd import _lib
    L = _lib.load()
    fn = L.eagle_spectral_settest

    def text():
        return L.eagle_open_error().decode()

    n, c, k = 8, 2, 2
    lam = (C.c_double * n)(*np.linspace(1.0, 2.0, n))
    UtX = (C.c_double * (n * c))(*np.arange(1.0, n * c + 1))
    Uty = (C.c_double * n)(*np.arange(float(n)))
    ptr, idx, om = (C.c_long * 3)(0, 2, 5), (C.c_long * 5)(0, 1, 2, 3, 4), (C.c_double * 5)(1.0, 0.0, 2.0, 1.0, 1.0)
    stat, info, score, cov = (C.c_double * (7 * k))(), (C.c_int32 * (2 * k))(), (C.c_double * 5)(), (C.c_double * 13)()
    names = ("lam", "UtX", "Uty", "c", "varE", "varG", "nsets", "ptr", "idx", "omega", "stat", "info", "score", "cov")
    good = [lam, UtX, Uty, c, 1.0, 1.0, k, ptr, idx, om, stat, info, score, cov]

    def call(**kw):
        a = list(good)
        for key, v in kw.items():
            a[names.index(key)] = v
        return fn(None, *a)

    def longs(*v):
        return (C.c_long * len(v))(*v)

    for key in ("lam", "UtX", "Uty", "ptr", "idx", "omega", "stat", "info"):
        assert call(**{key: None}) == ERR_ARG and text() == "spectral_settest: NULL argument", key
    for bad in (0, -1, 15):
        assert call(c=bad) == ERR_ARG and text() == "spectral_settest: c outside [1, 14]"
    assert call(nsets=-1) == ERR_ARG and text() == "spectral_settest: nsets is negative"
    for key in ("varE", "varG"):
        for bad in (float("nan"), float("inf")):
            assert call(**{key: bad}) == ERR_ARG and text() == "spectral_settest: varE or varG is not finite"
    for bad in (longs(1, 2, 5), longs(0, 3, 2), longs(0, -1, 5)):
        assert call(ptr=bad) == ERR_ARG and text() == "spectral_settest: set_ptr must start at 0 and not decrease"
    assert call(ptr=longs(0, 0, 5)) == ERR_ARG and text() == "spectral_settest: an empty set"
    assert call(ptr=longs(0, 5, 5)) == ERR_ARG and text() == "spectral_settest: an empty set"
    big_idx, big_om = (C.c_long * 66)(*range(66)), (C.c_double * 66)(*([1.0] * 66))
    assert call(ptr=longs(0, 1, 66), idx=big_idx, omega=big_om) == ERR_ARG
    assert text() == "spectral_settest: a set above SETTEST_MAX_MARKERS = 64 markers"
    for bad in (-1.0, float("nan"), float("inf"), -0.5):
        w = (C.c_double * 5)(1.0, 1.0, bad, 1.0, 1.0)
        assert call(omega=w) == ERR_ARG and text() == "spectral_settest: a negative or non-finite weight"
    assert call(idx=longs(0, 1, -1, 3, 4)) == ERR_ARG and text() == "spectral_settest: marker index out of range"
    assert call() == ERR_ARG and text() == "spectral_settest: no context"                 # nothing wrong but the context
    assert call(score=None, cov=None, c=14, nsets=0, ptr=longs(0)) == ERR_ARG and text() == "spectral_settest: no context"
    assert call(ptr=longs(0, 1, 65), idx=big_idx, omega=big_om, varE=-3.0) == ERR_ARG and text() == "spectral_settest: no context"   # 64: allowed
