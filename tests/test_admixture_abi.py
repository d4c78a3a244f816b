"""CPU: the C ABI of the admixture EM step without a device -- eagle_admixture_em is declared, exported and bound, section 1b''''v of
the header states the rule and lies between 1b''''iv and 1c, every argument error is decided before a context is needed (ctx == NULL:
the text comes through eagle_open_error), and the Python wrappers refuse malformed input before the library is called.  No device work."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
EPS = 1e-6


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_admixture_symbol_declared_exported_and_bound():
    from eagleeverything_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    assert re.search(r"\bint\s+eagle_admixture_em\s*\(\s*eagle_ctx\s*\*", txt), "eagle_admixture_em is not declared in include/eagle_hip.h"
    assert re.search(r"#define\s+EAGLE_ADMIX_EPS\s+1e-6\b", txt) and re.search(r"#define\s+EAGLE_ADMIX_KMAX\s+16\b", txt)
    assert hasattr(L, "eagle_admixture_em"), "libeaglehip.so does not export eagle_admixture_em"
    sig = _lib.SIGNATURES["eagle_admixture_em"]
    assert sig[0] is C.c_int and len(sig[1]) == 9
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_admix.hip" in makefile and "eagle_admix.o" in makefile
    kern = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_admix.hip")).read()
    code = re.sub(r"//.*", "", kern)
    for name in ("k_admix_f", "k_admix_q", "k_admix_ll_finish", "k_admix_q_finish", "__builtin_amdgcn_mfma_f64_16x16x4f64", "log("):
        assert name in code, name
    assert "asm" not in code and "atomic" not in code.lower()        # plain HIP with the MFMA builtin, no atomics of any kind
    ctxh = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ctx.h")).read()
    for name in ("eagle_dev_admix_window", "eagle_dev_admix_finish"):
        assert name in ctxh and hasattr(L, name)
    hosth = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_host.h")).read()
    assert "admix_range_plan" in hosth and "admix_part_cap" in hosth


def test_header_states_the_rule():
    txt = " ".join(header().replace("*", " ").split())
    assert txt.index("1b''''iv.") < txt.index("1b''''v.") < txt.index("1c.")
    sec = txt[txt.index("1b''''v."):txt.index("1c.")]
    for phrase in ("p_im = sum_k q_ik f_km", "pbar_im = sum_k q_ik (1 - f_km)", "p-bar is its own sum, never 1 - p",
                   "l(Q, F) = sum_m sum_i [ d ln p + (2 - d) ln pbar ]", "d = g + 1 copies of the allele that the character '2' stands for",
                   "a missing call of the source is a heterozygote", "A_im = d_im / p_im and B_im = (2 - d_im) / pbar_im",
                   "sa_km = f_km sum_i q_ik A_im", "sb_km = (1 - f_km) sum_i q_ik B_im", "f'_km = clamp(sa / (sa + sb), eps, 1 - eps)",
                   "f'_km = f_km where sa + sb = 0", "t_ik = q_ik sum_m (f_km A_im + (1 - f_km) B_im)", "q'_ik = max(t_ik / (2 L), eps)",
                   "every row of Q' is divided by its sum", "eps = EAGLE_ADMIX_EPS = 1e-6", "1 <= K <= EAGLE_ADMIX_KMAX = 16",
                   "Tang et al. 2005", "f' = clamp(mean(d) / 2)", "Q is n x K row-major, F is L x K row-major",
                   "loglik_out has steps + 1 entries: entry t is l at the parameters entering step t",
                   "the last entry is l at the returned parameters, from a likelihood-only pass of the same kernel",
                   "steps = 0 computes loglik_out[0] and returns Q and F untouched", "Individuals with index >= n do not exist",
                   "do not rely on the image's padding", "v_mfma_f64_16x16x4_f64", "k_admix_f", "k_admix_q", "admix_range_plan",
                   "part[S][n16][16]", "a function of (n, L) alone", "No atomics", "The same words on every route",
                   "a streamed window holds a multiple of 16 lines", "so do steps = 5 and five calls with steps = 1",
                   "Bit equality with the host restatement (r_api.admixture_host) is not claimed",
                   "Agreement with the ADMIXTURE or STRUCTURE programs is neither claimed nor tested", "a .bed route that skips missing calls",
                   "supervised mode", "cross-validation of K", "device-held state between calls", "sex chromosomes",
                   "a multi-device context works on its first device", "decided before the context is used", "n > 2^30 - 1",
                   "K outside [1, 16]", "steps outside [0, 10000]", "a non-finite Q or F entry", "an F entry outside [eps, 1 - eps]",
                   "a negative Q entry", "a Q row whose sum is off 1 by more than 1e-9"):
        assert phrase in sec, phrase
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "Admixture(" in readme and "add_ancestry" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.8r" in design and "k_admix_f" in design and "k_admix_q" in design
    assert os.path.exists(os.path.join(ROOT, "tools", "admixture_timing.py"))


def test_admixture_interface_is_public():
    import eagleeverything_amd
    from eagleeverything_amd import am, r_api, rcpp_api
    assert eagleeverything_amd.__all__ == ["rcpp_api", "r_api", "host_model", "synth"]
    p = inspect.signature(rcpp_api.admixture_em).parameters
    assert list(p)[:4] == ["f_name_ascii_Mt", "dims", "Q", "F"]
    assert [(k, p[k].default) for k in list(p)[4:]] == [("steps", 1), ("availmemGb", 8), ("device", 0)]
    p = inspect.signature(r_api.Admixture).parameters
    assert list(p)[:2] == ["geno", "K"]
    assert [(k, p[k].default) for k in list(p)[2:]] == [("seed", 0), ("tol", 1e-4), ("max_iter", 2000), ("accel", "squarem"), ("init", None),
                                                        ("availmemGb", 8), ("device", 0), ("step", None)]
    assert list(inspect.signature(r_api.admixture_host).parameters) == ["Mt8", "Q", "F", "steps"]
    p = inspect.signature(r_api.admixture_init).parameters
    assert list(p) == ["n", "L", "K", "seed", "freq"] and p["freq"].default is None
    assert list(inspect.signature(am.add_ancestry).parameters) == ["X", "adm"]
    assert (rcpp_api.ADMIX_EPS, rcpp_api.ADMIX_KMAX) == (EPS, 16)


def good_inputs(n=6, nm=9, K=3):
    rng = np.random.default_rng(0)
    Q = rng.dirichlet(np.ones(K), size=n)
    F = rng.uniform(0.1, 0.9, size=(nm, K))
    return Q, F


def test_python_wrappers_refuse_before_the_library(tmp_path, monkeypatch):
    from eagleeverything_amd import _lib, r_api, rcpp_api
    Mt = str(tmp_path / "Mt.ascii")
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    Q, F = good_inputs()

    def changed(A, i, j, v):
        B = A.copy()
        B[i, j] = v
        return B

    off = Q.copy()
    off[2] *= 1.0 + 1e-8
    bad = [dict(Q=Q[:5]), dict(Q=Q[:, 0]), dict(Q=np.ones((6, 17)) / 17), dict(Q=np.ones((6, 0))), dict(F=F[:8]), dict(F=F[:, :2]), dict(F=F.T),
           dict(Q=changed(Q, 0, 0, np.nan)), dict(Q=changed(Q, 0, 0, np.inf)), dict(F=changed(F, 0, 0, np.nan)), dict(F=changed(F, 8, 2, 0.0)),
           dict(F=changed(F, 8, 2, 1.0)), dict(F=changed(F, 3, 1, EPS / 2)), dict(Q=changed(changed(Q, 1, 0, -0.25), 1, 1, Q[1, 0] + Q[1, 1] + 0.25)),
           dict(Q=off), dict(Q=np.array([["a"] * 3] * 6)), dict(steps=-1), dict(steps=10001), dict(steps=1.5), dict(steps=True)]
    for kw in bad:
        args = dict(Q=Q, F=F, steps=1)
        args.update(kw)
        with pytest.raises(ValueError):
            rcpp_api.admixture_em(Mt, (6, 9), **args)
    geno = {"asciifileM": str(tmp_path / "M.ascii"), "asciifileMt": Mt, "dim_of_ascii_M": [6, 9]}
    for kw in (dict(K=0), dict(K=17), dict(K=2.5), dict(K=True), dict(accel="newton"), dict(tol=0.0), dict(max_iter=0), dict(init=(Q[:5], F)),
               dict(init=(Q, F), K=2), dict(init=(Q, changed(F, 0, 0, 0.0)))):
        args = dict(K=3, init=(Q, F))
        args.update(kw)
        with pytest.raises(ValueError):
            r_api.Admixture(geno, **args)


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib, rcpp_api
    L = _lib.load()
    fn = L.eagle_admixture_em

    def text():
        return L.eagle_open_error().decode()

    n, nm, K = 6, 9, 3
    Q, F = good_inputs(n, nm, K)
    dims, path = (C.c_long * 2)(n, nm), os.fsencode(str(tmp_path / "nothing"))
    c_dp = C.POINTER(C.c_double)

    def dp(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data_as(c_dp)

    keep = []
    ll = (C.c_double * 4)()
    good = [path, dims, K, 3, dp(Q), dp(F), 8.0, C.cast(ll, c_dp)]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[("path", "dims", "K", "steps", "Q", "F", "mem", "ll").index(k)] = v
        return fn(None, *a)

    def changed(A, i, j, v):
        B = A.copy()
        B[i, j] = v
        return B

    for k in ("path", "dims", "Q", "F", "ll"):
        assert call(**{k: None}) == ERR_ARG and text() == "admixture_em: NULL argument", k
    for bad in ((0, nm), (n, 0), (-1, nm)):
        assert call(dims=(C.c_long * 2)(*bad)) == ERR_ARG and text() == "admixture_em: dims must be positive"
    assert call(dims=(C.c_long * 2)(1 << 30, nm)) == ERR_ARG and "2^30 - 1" in text()        # before a single entry is read
    for bad in (0, -1, 17):
        assert call(K=bad) == ERR_ARG and text() == "admixture_em: K outside [1, 16]"
    for bad in (-1, 10001):
        assert call(steps=bad) == ERR_ARG and text() == "admixture_em: steps outside [0, 10000]"
    for bad in (float("nan"), float("inf")):
        assert call(Q=dp(changed(Q, 5, 2, bad))) == ERR_ARG and text() == "admixture_em: a non-finite Q entry"
        assert call(F=dp(changed(F, 8, 2, bad))) == ERR_ARG and text() == "admixture_em: a non-finite F entry"
    for bad in (0.0, 1.0, EPS * 0.999, -0.5, 1.5):
        assert call(F=dp(changed(F, 4, 1, bad))) == ERR_ARG and text() == "admixture_em: an F entry outside [eps, 1 - eps]"
    neg = changed(changed(Q, 1, 0, -0.25), 1, 1, Q[1, 0] + Q[1, 1] + 0.25)                  # the row still sums to 1
    assert call(Q=dp(neg)) == ERR_ARG and text() == "admixture_em: a negative Q entry"
    for scale in (1.0 + 1e-8, 1.0 - 1e-8, 0.0):
        off = Q.copy()
        off[3] *= scale
        assert call(Q=dp(off)) == ERR_ARG and text() == "admixture_em: a Q row whose sum is off 1 by more than 1e-9"
    edge = F.copy()
    edge[0], edge[1] = EPS, 1.0 - EPS                                                        # the ends of the interval are inside it
    unit = Q.copy()
    unit[0] = (1.0, 0.0, 0.0)
    assert call(F=dp(edge), Q=dp(unit)) == ERR_ARG and text() == "admixture_em: no context"
    assert call() == ERR_ARG and text() == "admixture_em: no context"                        # nothing wrong but the context
    assert call(steps=0) == ERR_ARG and text() == "admixture_em: no context"
    assert call(steps=10000, K=3) == ERR_ARG and text() == "admixture_em: no context"
    import torch
    if not torch.cuda.is_available():
        assert not rcpp_api._ctx                                                             # and no device was opened on the way
