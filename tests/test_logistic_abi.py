"""CPU: the C ABI of the logistic regression without a device -- eagle_logistic is declared, exported and bound, section 1b''''iv of
the header states the model, the rule and the codes and lies between 1b''''iii and 1c, every argument error is decided before a
context is needed (ctx == NULL: the text comes through eagle_open_error), and the Python wrappers refuse malformed input before
the library is called.  No device work."""
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


def test_logistic_symbol_declared_exported_and_bound():
    from eagleeverything_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    assert re.search(r"\bint\s+eagle_logistic\s*\(\s*eagle_ctx\s*\*", txt), "eagle_logistic is not declared in include/eagle_hip.h"
    assert hasattr(L, "eagle_logistic"), "libeaglehip.so does not export eagle_logistic"
    sig = _lib.SIGNATURES["eagle_logistic"]
    assert sig[0] is C.c_int and len(sig[1]) == 13
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_logit.hip" in makefile and "eagle_logit.o" in makefile
    kern = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_logit.hip")).read()
    code = re.sub(r"//.*", "", kern)
    assert "k_logit_irls" in code and "__builtin_amdgcn_mfma_f64_16x16x4f64" in code and "log1p" in code and "exp(" in code
    assert "asm" not in code and "atomic" not in code.replace("__ATOMIC_", "")        # the fence's memory-order constants are no atomics
    assert "__syncthreads" not in code                                                 # the waves of a workgroup never meet
    ctxh = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ctx.h")).read()
    assert "eagle_dev_logistic" in ctxh and hasattr(L, "eagle_dev_logistic")


def test_header_states_the_rule():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b''''iv."):txt.index("1c.")]
    for phrase in ("logit P(y_i = 1) = x_i' beta + g_im gamma", "-1 = not used", "the caller supplies the intercept column",
                   "1 <= c <= 15, so p = c + 1 <= 16", "the image value plus one", "the allele whose odds ratio CaseControl reports",
                   "r_api.logistic_host", "Every fit starts at (beta0, 0)", "r_api.logistic_null_host",
                   "mu_i = 1 / (1 + e^-eta_i), w_i = mu_i (1 - mu_i)", "U = sum (y_i - mu_i) x~_i", "I = sum w_i x~_i x~_i'",
                   "l = sum [y_i eta_i - log(1 + e^eta_i)]", "score = U_g^2 (I^-1)_gg", "N num^2 / (R S tvar)",
                   "scale delta so that max |delta_j| <= 5", "stop when max_j |delta_j| <= tol", "at most max_iter evaluations",
                   "Heinze and Schemper 2002", "h_i = w_i x~_i' I^-1 x~_i", "U _j = sum [y_i - mu_i + h_i (1/2 - mu_i)] x~_ij",
                   "no step halving", "takes two passes over the individuals", "as PLINK 2 does",
                   "the penalised likelihood-ratio test is not reported", "stat_out[4 m ..] = (gamma, se = sqrt((I^-1)_gg), score, l)",
                   "info_out[2 m ..] = (code, evaluations", "0 converged; 1 max_iter reached; 2 a Cholesky pivot of I was not positive or not finite",
                   "3 separation (ML only)", "max_i |eta_i| > 40", "+ 256 the value reported is the Firth fit",
                   "NaN unless the code's low byte is 0", "score is NaN only under code 2 at the first evaluation",
                   "restarted from (beta0, 0) with Firth, in the same kernel and by the same wave", "v_mfma_f64_16x16x4_f64",
                   "Agreement with the PLINK or logistf programs is neither claimed nor tested", "Bit equality with the host restatement is not claimed",
                   "one entry per kept individual", "a multi-device context works on its first device", "decided before the context is used",
                   "n > 2^30 - 1", "c outside [1, 15]", "a status outside {-1, 0, 1}", "firth outside {0, 1, 2}", "tol not in (0, 1)",
                   "max_iter outside [1, 1000]", "no case or no control among the used individuals"):
        assert phrase in sec, phrase
    assert txt.index("1b''''iii.") < txt.index("1b''''iv.") < txt.index("1c.")
    old = txt[txt.index("1b''''iii."):txt.index("1b''''iv.")]
    assert "Logistic regression with covariates is section 1b''''iv" in old
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "Logistic(" in readme and "not timed" in readme and "impute=" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.8p" in design and "k_logit_irls" in design
    assert os.path.exists(os.path.join(ROOT, "tools", "logistic_timing.py"))


def test_logistic_interface_is_public():
    import eagleeverything_amd
    from eagleeverything_amd import r_api, rcpp_api
    assert eagleeverything_amd.__all__ == ["rcpp_api", "r_api", "host_model", "synth"]
    p = inspect.signature(rcpp_api.logistic).parameters
    assert [(k, p[k].default) for k in list(p)[4:]] == [("beta0", None), ("firth", 2), ("tol", 1e-10), ("max_iter", 50), ("availmemGb", 8),
                                                        ("device", 0)]
    assert list(p)[:4] == ["f_name_ascii_Mt", "dims", "status", "X"]
    p = inspect.signature(r_api.Logistic).parameters
    assert [(k, p[k].default) for k in list(p)[2:]] == [("X", None), ("firth", "fallback"), ("tol", 1e-10), ("max_iter", 50), ("availmemGb", 8),
                                                        ("device", 0)]
    assert list(inspect.signature(r_api.logistic_host).parameters)[:6] == ["Mt8", "status", "X", "firth", "tol", "max_iter"]
    assert list(inspect.signature(r_api.logistic_null_host).parameters)[:2] == ["X", "y"]
    p = inspect.signature(r_api.CaseControl).parameters                                   # left alone
    assert [(k, p[k].default) for k in list(p)[2:4]] == [("bed", None), ("fisher", False)]


def test_python_wrappers_refuse_before_the_library(tmp_path, monkeypatch):
    from eagleeverything_amd import _lib, r_api, rcpp_api
    Mt = str(tmp_path / "Mt.ascii")
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    st = [0, 1, -1, 0, 1, 1]
    X = np.column_stack([np.ones(6), np.arange(6.0)])
    nanX = X.copy()
    nanX[0, 1] = np.nan
    bad = [dict(status=[0, 1, 0]), dict(status=[0, 1, 2, 0, 1, 1]), dict(status=[0, 0.5, 1, 0, 1, 1]), dict(status=[[0, 1, 0], [1, 0, 1]]),
           dict(status=[0, 0, -1, 0, 0, 0]), dict(status=[1, 1, -1, 1, 1, 1]), dict(status=["a"] * 6), dict(X=np.ones((5, 1))), dict(X=np.ones(6)),
           dict(X=np.ones((6, 16))), dict(X=np.ones((6, 0))), dict(X=nanX), dict(firth=3), dict(firth=-1), dict(tol=0.0), dict(tol=1.0),
           dict(tol=float("nan")), dict(max_iter=0), dict(max_iter=1001), dict(max_iter=2.5), dict(beta0=[0.0]), dict(beta0=[0.0, float("inf")])]
    for kw in bad:
        args = dict(status=st, X=X, beta0=[0.0, 0.0])
        args.update(kw)
        with pytest.raises(ValueError):
            rcpp_api.logistic(Mt, (6, 4), **args)
    geno = {"asciifileM": str(tmp_path / "M.ascii"), "asciifileMt": Mt, "dim_of_ascii_M": [6, 4]}
    for kw in (dict(status=[0, 1, 0]), dict(status=[0, 1, 2, 0, 1, 1]), dict(status=[0, 0, None, 0, 0, 0]), dict(X=np.ones((5, 1))),
               dict(X=np.ones((6, 16))), dict(firth="sometimes"), dict(X=np.column_stack([np.ones(6), [0, np.inf, 0, 0, 0, 0]])),
               dict(status=[1, 0, None, 0, 0, 0], X=np.column_stack([np.ones(6), [np.nan, 0, 1, 2, 3, 4]]))):       # the NaN drops the only case
        args = dict(status=[0, 1, float("nan"), 0, 1, 1], X=None)
        args.update(kw)
        with pytest.raises(ValueError):
            r_api.Logistic(geno, **args)


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib, rcpp_api
    L = _lib.load()
    fn = L.eagle_logistic

    def text():
        return L.eagle_open_error().decode()

    n, nm, c = 6, 9, 2
    dims, path = (C.c_long * 2)(n, nm), os.fsencode(str(tmp_path / "nothing"))
    st = (C.c_int32 * n)(0, 1, -1, 0, 1, 1)
    X = (C.c_double * (n * c))(1, 1, 1, 1, 1, 1, 0.5, -1, float("nan"), 2, 3, 4)          # the NaN belongs to the unused individual
    b0 = (C.c_double * c)(0.1, 0.2)
    stat, info = (C.c_double * (4 * nm))(), (C.c_int32 * (2 * nm))()
    good = [path, dims, st, X, c, b0, 2, 1e-10, 50, 8.0, stat, info]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[("path", "dims", "st", "X", "c", "b0", "firth", "tol", "max_iter", "mem", "stat", "info").index(k)] = v
        return fn(None, *a)

    for k in ("path", "dims", "st", "X", "b0", "stat", "info"):
        assert call(**{k: None}) == ERR_ARG and text() == "logistic: NULL argument", k
    for bad in ((0, nm), (n, 0), (-1, nm)):
        assert call(dims=(C.c_long * 2)(*bad)) == ERR_ARG and text() == "logistic: dims must be positive"
    assert call(dims=(C.c_long * 2)(1 << 30, nm)) == ERR_ARG and "2^30 - 1" in text()      # before a single status is read
    for bad in (0, -1, 16):
        assert call(c=bad) == ERR_ARG and text() == "logistic: c outside [1, 15]"
    for bad in (-1, 3):
        assert call(firth=bad) == ERR_ARG and text() == "logistic: firth outside {0, 1, 2}"
    for bad in (0.0, 1.0, -1e-3, float("nan")):
        assert call(tol=bad) == ERR_ARG and text() == "logistic: tol not in (0, 1)"
    for bad in (0, 1001, -5):
        assert call(max_iter=bad) == ERR_ARG and text() == "logistic: max_iter outside [1, 1000]"
    for bad in (2, -2):
        assert call(st=(C.c_int32 * n)(0, 1, -1, 0, bad, 1)) == ERR_ARG and text() == "logistic: a status outside {-1, 0, 1}"
    assert call(X=(C.c_double * (n * c))(1, 1, 1, 1, 1, 1, 0.5, float("inf"), 0, 2, 3, 4)) == ERR_ARG and "non-finite X entry" in text()
    assert call(X=(C.c_double * (n * c))(1, 1, 1, 1, 1, float("nan"), 0.5, 1, 0, 2, 3, 4)) == ERR_ARG and "non-finite X entry" in text()
    assert call(b0=(C.c_double * c)(0.1, float("nan"))) == ERR_ARG and "non-finite beta0" in text()
    assert call(st=(C.c_int32 * n)(0, 0, -1, 0, 0, 0)) == ERR_ARG and text() == "logistic: no case or no control among the used individuals"
    assert call(st=(C.c_int32 * n)(1, 1, -1, 1, -1, 1)) == ERR_ARG and "no case or no control" in text()
    assert call() == ERR_ARG and text() == "logistic: no context"                         # nothing wrong but the context
    assert call(firth=0, max_iter=1000, tol=0.5) == ERR_ARG and text() == "logistic: no context"
    # through the wrapper an argument error of the library arrives as EagleError(-3) and opens no device
    import torch
    if not torch.cuda.is_available():
        assert not rcpp_api._ctx
    with pytest.raises(rcpp_api.EagleError) as e:
        rcpp_api.logistic(str(tmp_path / "nothing"), (6, 0), [0, 1, -1, 0, 1, 1], np.ones((6, 1)), beta0=[0.0])
    assert e.value.code == ERR_ARG and "dims must be positive" in e.value.text
