"""CPU: the C ABI of the saddlepoint call without a device -- eagle_glmm_spa is declared, exported and bound, section 1d''' of the header
states the rule and the codes and lies between 1d'' and section 2, every argument error is decided before a context is needed
(ctx == NULL: the text comes through eagle_open_error), and the Python wrappers refuse malformed input before the library is called.
No device work."""
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


def test_glmm_symbol_declared_exported_and_bound():
    from eagleeverything_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    assert re.search(r"\bint\s+eagle_glmm_spa\s*\(\s*eagle_ctx\s*\*", txt), "eagle_glmm_spa is not declared in include/eagle_hip.h"
    assert hasattr(L, "eagle_glmm_spa"), "libeaglehip.so does not export eagle_glmm_spa"
    sig = _lib.SIGNATURES["eagle_glmm_spa"]
    assert sig[0] is C.c_int and len(sig[1]) == 15
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_glmm.hip" in makefile and "eagle_glmm.o" in makefile
    kern = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_glmm.hip")).read()
    code = re.sub(r"//.*", "", kern)
    assert "k_glmm_spa" in code and "__builtin_amdgcn_mfma_f64_16x16x4f64" in code and "log1p" in code and "exp(" in code
    assert "asm" not in code and "atomic" not in code.replace("__ATOMIC_", "")        # the fence's memory-order constants are no atomics
    assert "__syncthreads" not in code                                                 # the waves of a workgroup never meet
    ctxh = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ctx.h")).read()
    assert "eagle_dev_glmm_spa" in ctxh and hasattr(L, "eagle_dev_glmm_spa")


def test_header_states_the_rule():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1d'''."):txt.index(" 2. Device-resident entry points")]
    for phrase in ("logit mu_i = x_i' alpha + b_i, b ~ N(0, tau K)", "Chen et al. 2016", "Dey et al. 2017, Zhou et al. 2018", "glmm.spa_host",
                   "the caller supplies the intercept column, 1 <= c <= 15", "A = (X'DX)^-1", "or NULL for V = V ", "the image value plus one",
                   "y - mu = P Y and X'(y - mu) = 0", "s = X'D g, beta = A s, G~_i = g_i - x_i' beta", "T = sum g_i resid_i",
                   "V = sum D_i G~_i^2", "m = sum G~_i mu_i", "V <= 2^-40 sum D_i g_i^2", "a V that is not finite and positive",
                   "z = T / sqrt(V), q = z sqrt(V ) = T sqrt(V / V)", "code 4 and 0 evaluations", "SAIGE's cutoff is 2",
                   "K(t) = sum log(1 - mu_i + mu_i e^(t G~_i)) - t m", "K'(t) = sum mu_i G~_i / ((1 - mu_i) e^(-t G~_i) + mu_i) - m",
                   "K''(t) = sum (1 - mu_i) mu_i G~_i^2 e^(-t G~_i) / ((1 - mu_i) e^(-t G~_i) + mu_i)^2", "e = exp(-|a|), u = 1 - e, den = 1 - nu u",
                   "nu |a| + log1p(-nu u)", "sign(a) D_i G~_i u / den", "D_i G~_i^2 e / den^2", "one exp and one log1p",
                   "K'(0) = 0 and K''(0) = V need no evaluation", "zeta_max = 500 / max_i |G~_i|", "by more than 2^-40 |target|",
                   "An unreachable observed-side target is code 3", "contributes no probability and sets + 256", "by Newton from zeta = 0",
                   "bisect when the step leaves the bracket", "the bracket is updated by the sign of K' - target",
                   "stop when |delta zeta| sqrt(V ) <= tol", "at most max_iter evaluations per tail", "The first code that is not 0 ends the marker",
                   "w = sign(zeta) sqrt(2 (zeta target - K(zeta))), v = zeta sqrt(K''(zeta)), r = w + ln(v / w) / w",
                   "where |zeta| sqrt(V ) < 10^-4, r = target / sqrt(V )", "stat_out[7 m ..] = (T, V , z, zeta_up, r _up, zeta_lo, r _lo)",
                   "info_out[2 m ..] = (code, evaluations", "0 both tails solved; 1 max_iter reached; 2 degenerate; 3 observed-side target unreachable; 4 below the cutoff",
                   "+ 256 the opposite tail was unreachable", "NaN unless the code's low byte is 0", "p_spa = Phi(-r _up) + Phi(r _lo)",
                   "k_glmm_spa", "v_mfma_f64_16x16x4_f64", "recomputes G~_i at every evaluation", "no barrier between waves and no atomics",
                   "Agreement with the GMMAT, SAIGE or SPAtest programs is neither claimed nor tested", "Bit equality with the numpy restatement is not claimed",
                   "a multi-device context works on its first device", "decided before the context is used", "n > 2^30 - 1", "c outside [1, 15]",
                   "a mu outside (0, 1) or not finite", "a non-finite X, resid or A entry", "cutoff < 0 or NaN", "tol not in (0, 1)",
                   "max_iter outside [1, 1000]"):
        assert phrase in sec, phrase
    assert txt.index("1d''.") < txt.index("1d'''.") < txt.index(" 2. Device-resident entry points")
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "GLMM(" in readme and "saddlepoint" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.8w" in design and "k_glmm_spa" in design and "d_p4" in design
    assert os.path.exists(os.path.join(ROOT, "tools", "glmm_timing.py"))


def test_glmm_interface_is_public():
    import eagleeverything_amd
    from eagleeverything_amd import glmm, r_api, rcpp_api
    assert eagleeverything_amd.__all__ == ["rcpp_api", "r_api", "host_model", "synth"]
    assert "glmm" in eagleeverything_amd.__doc__
    want = [("X", None), ("tau", None), ("spa_cutoff", 2.0), ("tol", 1e-10), ("max_iter", 50), ("map", None), ("backend", None), ("availmemGb", 8),
            ("device", 0)]
    for fn in (glmm.GLMM, r_api.GLMM):
        p = inspect.signature(fn).parameters
        assert list(p)[:2] == ["geno", "status"] and [(k, p[k].default) for k in list(p)[2:]] == want
    p = inspect.signature(glmm.spa).parameters
    assert list(p)[:5] == ["f_name_ascii_Mt", "dims", "mu", "resid", "X"]
    assert [(k, p[k].default) for k in list(p)[5:]] == [("A", None), ("vara", None), ("cutoff", 2.0), ("tol", 1e-10), ("max_iter", 50),
                                                        ("availmemGb", 8), ("device", 0)]
    assert list(inspect.signature(glmm.spa_host).parameters)[:4] == ["Mt8", "mu", "resid", "X"]
    p = inspect.signature(glmm.null_fit).parameters
    assert [(k, p[k].default) for k in list(p)[3:]] == [("tau", None), ("tol", 1e-6), ("max_iter", 100)] and list(p)[:3] == ["y", "X", "K"]
    # the wrapper is glmm's: rcpp_api's public functions each have a case in tests/test_gpu_poison.py, and that table is not this one's
    assert not any("glmm" in k.lower() or k == "spa" for k in vars(rcpp_api))


def test_python_wrappers_refuse_before_the_library(tmp_path, monkeypatch):
    from eagleeverything_amd import _lib, glmm, r_api
    Mt = str(tmp_path / "Mt.ascii")
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    n = 6
    mu, r = np.full(n, 0.3), np.array([0.7, -0.3, -0.3, 0.7, -0.3, -0.3])
    X = np.column_stack([np.ones(n), np.arange(6.0)])
    nanX = X.copy()
    nanX[0, 1] = np.nan
    bad = [dict(mu=mu[:5]), dict(mu=np.r_[mu[:5], 0.0]), dict(mu=np.r_[mu[:5], 1.0]), dict(mu=np.r_[mu[:5], np.nan]), dict(mu=["a"] * 6),
           dict(mu=mu.reshape(2, 3)), dict(resid=r[:5]), dict(resid=np.r_[r[:5], np.inf]), dict(X=np.ones((5, 1))), dict(X=np.ones(6)),
           dict(X=np.ones((6, 16))), dict(X=np.ones((6, 0))), dict(X=nanX), dict(A=np.eye(3)), dict(A=[[1.0, 0.0], [0.0, np.nan]]),
           dict(X=np.ones((6, 2))), dict(vara=np.ones(3)), dict(cutoff=-1.0), dict(cutoff=float("nan")), dict(tol=0.0), dict(tol=1.0),
           dict(tol=float("nan")), dict(max_iter=0), dict(max_iter=1001), dict(max_iter=2.5)]
    for kw in bad:
        args = dict(mu=mu, resid=r, X=X)
        args.update(kw)
        with pytest.raises(ValueError):
            glmm.spa(Mt, (6, 4), **args)
    with pytest.raises(ValueError):
        glmm.spa(Mt, (6, 0), mu, r, X)
    geno = {"asciifileM": str(tmp_path / "M.ascii"), "asciifileMt": Mt, "dim_of_ascii_M": [6, 4]}
    for kw in (dict(status=[0, 1, 0]), dict(status=[0, 1, 2, 0, 1, 1]), dict(status=[0, 0, None, 0, 0, 0]), dict(status=["a"] * 6),
               dict(X=np.ones((5, 1))), dict(X=np.ones((6, 16))), dict(X=np.column_stack([np.ones(6), [0, np.inf, 0, 0, 0, 0]])),
               dict(status=[1, 0, None, 0, 0, 0], X=np.column_stack([np.ones(6), [np.nan, 0, 1, 2, 3, 4]])),   # the NaN drops the only case
               dict(tau=-1.0), dict(tau=1e-9), dict(spa_cutoff=-0.5), dict(tol=2.0), dict(max_iter=0)):
        args = dict(status=[0, 1, float("nan"), 0, 1, 1], X=None)
        args.update(kw)
        for fn in (glmm.GLMM, r_api.GLMM):
            with pytest.raises(ValueError):
                fn(geno, **args)
    with pytest.raises(TypeError):
        r_api.GLMM(geno, [0, 1, 0, 0, 1, 1], Zmat=np.eye(6))                  # repeated measures are not supported


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib, glmm, rcpp_api
    L = _lib.load()
    fn = L.eagle_glmm_spa

    def text():
        return L.eagle_open_error().decode()

    n, nm, c = 6, 9, 2
    dims, path = (C.c_long * 2)(n, nm), os.fsencode(str(tmp_path / "nothing"))
    mu = (C.c_double * n)(*([0.3] * n))
    res = (C.c_double * n)(0.7, -0.3, -0.3, 0.7, -0.3, -0.3)
    X = (C.c_double * (n * c))(1, 1, 1, 1, 1, 1, 0.5, -1, 0, 2, 3, 4)
    A = (C.c_double * (c * c))(1, 0, 0, 1)
    vara = (C.c_double * nm)(*([1.0] * nm))
    stat, info = (C.c_double * (7 * nm))(), (C.c_int32 * (2 * nm))()
    names = ("path", "dims", "mu", "res", "X", "c", "A", "vara", "cutoff", "tol", "max_iter", "mem", "stat", "info")
    good = [path, dims, mu, res, X, c, A, vara, 2.0, 1e-10, 50, 8.0, stat, info]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(None, *a)

    for k in ("path", "dims", "mu", "res", "X", "A", "stat", "info"):
        assert call(**{k: None}) == ERR_ARG and text() == "glmm_spa: NULL argument", k
    for bad in ((0, nm), (n, 0), (-1, nm)):
        assert call(dims=(C.c_long * 2)(*bad)) == ERR_ARG and text() == "glmm_spa: dims must be positive"
    assert call(dims=(C.c_long * 2)(1 << 30, nm)) == ERR_ARG and "2^30 - 1" in text()      # before a single mu is read
    for bad in (0, -1, 16):
        assert call(c=bad) == ERR_ARG and text() == "glmm_spa: c outside [1, 15]"
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        assert call(mu=(C.c_double * n)(0.3, 0.3, bad, 0.3, 0.3, 0.3)) == ERR_ARG and text() == "glmm_spa: a mu outside (0, 1)", bad
    assert call(res=(C.c_double * n)(0.7, float("nan"), -0.3, 0.7, -0.3, -0.3)) == ERR_ARG and "non-finite resid entry" in text()
    assert call(X=(C.c_double * (n * c))(1, 1, 1, 1, 1, 1, 0.5, float("inf"), 0, 2, 3, 4)) == ERR_ARG and "non-finite X entry" in text()
    assert call(A=(C.c_double * (c * c))(1, 0, float("nan"), 1)) == ERR_ARG and "non-finite A entry" in text()
    for bad in (-1e-3, float("nan")):
        assert call(cutoff=bad) == ERR_ARG and text() == "glmm_spa: cutoff negative or NaN"
    for bad in (0.0, 1.0, -1e-3, float("nan")):
        assert call(tol=bad) == ERR_ARG and text() == "glmm_spa: tol not in (0, 1)"
    for bad in (0, 1001, -5):
        assert call(max_iter=bad) == ERR_ARG and text() == "glmm_spa: max_iter outside [1, 1000]"
    assert call() == ERR_ARG and text() == "glmm_spa: no context"                         # nothing wrong but the context
    assert call(vara=None, cutoff=0.0, max_iter=1000, tol=0.5) == ERR_ARG and text() == "glmm_spa: no context"
    # through the wrapper an argument error of the library arrives as EagleError(-3) and opens no device
    import torch
    if not torch.cuda.is_available():
        assert not rcpp_api._ctx
    with pytest.raises(rcpp_api.EagleError) as e:                                         # what glmm.spa calls the library through
        rcpp_api._args_first(fn, 0, tuple(good[:1] + [(C.c_long * 2)(n, 0)] + good[2:]))
    assert e.value.code == ERR_ARG and "dims must be positive" in e.value.text
    if not torch.cuda.is_available():
        assert not rcpp_api._ctx
    assert "_args_first(L.eagle_glmm_spa" in inspect.getsource(glmm.spa)
