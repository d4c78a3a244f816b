"""CPU: the C ABI of the max(T) permutation pass without a device -- eagle_maxt is declared, exported and bound, section 1b''''vi of the
header states the rule, every argument error is decided before a context is needed (ctx == NULL: EAGLE_ERR_ARG with its text through
eagle_open_error), and the Python wrappers refuse malformed input before the library is called.  No device work."""
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


def test_maxt_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    assert re.search(r"\bint\s+eagle_maxt\s*\(\s*eagle_ctx\s*\*", txt) and hasattr(L, "eagle_maxt")
    assert _lib.SIGNATURES["eagle_maxt"][0] is C.c_int and len(_lib.SIGNATURES["eagle_maxt"][1]) == 17
    for name, val in (("EAGLE_MAXT_MAX_N", 65535), ("EAGLE_MAXT_TMAX", 1000000), ("EAGLE_MAXT_RMAX", 1024)):
        assert re.search(r"#define %s %dL?\b" % (name, val), txt), name
    assert (rcpp_api.MAXT_MAX_N, rcpp_api.MAXT_TMAX, rcpp_api.MAXT_RMAX) == (65535, 1000000, 1024)
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_maxt.hip" in makefile and "eagle_maxt.o" in makefile
    code = re.sub(r"//.*", "", open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_maxt.hip")).read())
    for k in ("k_maxt_keys", "k_maxt_sort_local", "k_maxt_sort_global", "k_maxt_operand", "k_maxt_tile", "k_maxt_finish",
              "__builtin_amdgcn_mfma_i32_32x32x32_i8", "__dmul_rn", "__ddiv_rn", "maxt_key64", "maxt_digits"):
        assert k in code, k
    assert "asm" not in code
    ctxh = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ctx.h")).read()
    for name in ("eagle_dev_maxt_permutations", "eagle_dev_maxt_operand", "eagle_dev_maxt_tile", "eagle_dev_maxt_finish", "eagle_dev_maxt_width"):
        assert name in ctxh and hasattr(L, name), name
    L.eagle_dev_maxt_width.restype, L.eagle_dev_maxt_width.argtypes = C.c_int, [C.c_int]
    assert [L.eagle_dev_maxt_width(P) for P in (1, 2, 3)] == [128, 64, 64]


def test_header_states_the_rule():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b''''vi."):txt.index("1c.")]
    for phrase in ("|t_i| <= EAGLE_MAXT_TMAX = 10^6", "u_0 < ... < u_{N-1}", "n <= EAGLE_MAXT_MAX_N = 65,535; 3 <= N", "first + R <= 2^31",
                   "V_m = N Q_m - S_m^2", "W = N sum t^2 - T^2", "d_m(t') = N c_m - S_m T", "< 2^53", "N^2 < 2^32",
                   "key_m(t') = fl(fl(d d) / V_m)", "key = 0 where V_m = 0", "counter = r 2^16 + j + 1", "0x9E3779B97F4A7C15",
                   "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "h has 32 bits", "N^2 / 2^33", "key64(r, j) = (strata[u_j] << 48) | (h << 16) | j",
                   "t^(r)[u_sigma[k]] = t[u_pi_r[k]]", "t^(r)[u_k] = t[u_perm[r - first][k]]", "the lowest m that attains it",
                   "add up to one call over [1, R]", "c = c_0 + 128 c_1 + 16384 c_2", "digit = sign(t) m_p in [-127, 127]",
                   "Agreement with the PLINK program is neither claimed nor tested", "decided before the context is used"):
        assert phrase in sec, phrase
    assert txt.index("1b''''v.") < txt.index("1b''''vi.") < txt.index("1c.")
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "MaxT" in readme and "max(T)" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k_maxt_tile" in design


def test_maxt_interface_is_public():
    import eagleeverything_amd
    from eagleeverything_amd import r_api, rcpp_api
    assert "MaxT" in eagleeverything_amd.__doc__
    for name in ("MaxT", "maxt_host", "maxt_permutations_host", "maxt_merge", "maxt_from_raw", "maxt_trait"):
        assert callable(getattr(r_api, name)), name
    p = inspect.signature(rcpp_api.maxt).parameters
    assert [(k, p[k].default) for k in list(p)[3:]] == [("used", None), ("strata", None), ("seed", 0), ("first", 1), ("R", 1000), ("perm", None),
                                                        ("availmemGb", 8), ("device", 0)]
    p = inspect.signature(r_api.MaxT).parameters
    assert [(k, p[k].default) for k in list(p)[2:8]] == [("R", 1000), ("seed", 0), ("within", None), ("kind", "auto"), ("availmemGb", 8), ("device", 0)]
    assert list(inspect.signature(r_api.maxt_host).parameters) == ["Mt8", "t", "used", "strata", "seed", "first", "R", "perm"]
    assert list(inspect.signature(r_api.maxt_permutations_host).parameters) == ["N", "strata_used", "seed", "first", "R"]


def test_python_wrappers_refuse_before_the_library(tmp_path, monkeypatch):
    from eagleeverything_amd import _lib, r_api, rcpp_api
    Mt = str(tmp_path / "Mt.ascii")
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    good = [0, 1, 0, 1, 1, 0]
    for kw in (dict(t=[0, 1, 0]), dict(t=[0, 0.5, 1, 0, 1, 0]), dict(t=[[0, 1, 0], [1, 0, 1]]), dict(t=good, used=[1, 1, 1]),
               dict(t=good, strata=[0, 1]), dict(t=good, strata=[0, 1, 0.5, 1, 0, 1]), dict(t=good, R=2, perm=[[0, 1, 2, 3, 4, 5]]),
               dict(t=good, R=1, perm=[[0, 1, 2, 3, 4]]), dict(t=good, R=1, perm=[[0.5, 1, 2, 3, 4, 5]]), dict(t=["a"] * 6)):
        with pytest.raises(ValueError):
            rcpp_api.maxt(Mt, (6, 4), **kw)
    geno = {"asciifileM": str(tmp_path / "M.ascii"), "asciifileMt": Mt, "dim_of_ascii_M": [6, 4]}
    for kw in (dict(trait=[0, 1, 0]), dict(trait=[1, 1, 1, 1, 1, 1]), dict(trait=good, R=0), dict(trait=good, first=0),
               dict(trait=[0, 1, np.nan, np.nan, np.nan, np.nan]), dict(trait=good, within=[1, 2, 3])):
        with pytest.raises(ValueError):
            r_api.MaxT(geno, **kw)


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib, rcpp_api
    L = _lib.load()
    n, nm, R = 6, 9, 2
    i32 = lambda *v: (C.c_int32 * len(v))(*v)                                # noqa: E731
    base = dict(path=os.fsencode(str(tmp_path / "nothing")), dims=(C.c_long * 2)(n, nm), t=i32(0, 1, 5, -3, 1, 1), used=None, strata=None,
                seed=7, first=1, R=R, perm=None, mem=8.0, d=(C.c_int64 * nm)(), V=(C.c_int64 * nm)(), k=(C.c_double * nm)(),
                c=(C.c_int32 * nm)(), mk=(C.c_double * R)(), am=(C.c_int32 * R)())

    def call(**kw):
        a = dict(base, **kw)
        rc = L.eagle_maxt(None, *[a[k] for k in ("path", "dims", "t", "used", "strata", "seed", "first", "R", "perm", "mem", "d", "V", "k", "c", "mk", "am")])
        return rc, L.eagle_open_error().decode()

    for k in ("path", "dims", "t", "d", "V", "k", "c", "mk", "am"):
        assert call(**{k: None}) == (ERR_ARG, "maxt: NULL argument"), k
    for bad in ((0, nm), (n, 0), (-1, nm)):
        assert call(dims=(C.c_long * 2)(*bad)) == (ERR_ARG, "maxt: dims must be positive")
    rc, text = call(dims=(C.c_long * 2)(65536, nm))                          # decided before a single trait value is read
    assert rc == ERR_ARG and "65535 individuals" in text
    u8 = lambda *v: (C.c_uint8 * len(v))(*v)                                 # noqa: E731
    rc, text = call(used=u8(1, 0, 0, 1, 0, 0))
    assert rc == ERR_ARG and "fewer than 3 used" in text
    rc, text = call(dims=(C.c_long * 2)(2, nm))
    assert rc == ERR_ARG and "fewer than 3 used" in text
    for v in (1000001, -1000001):
        rc, text = call(t=i32(0, 1, v, -3, 1, 1))
        assert rc == ERR_ARG and "EAGLE_MAXT_TMAX" in text
    assert call(t=i32(0, 1, 1000001, -3, 1, 1), used=u8(1, 1, 0, 1, 1, 1))[1] == "maxt: no context"      # an unused record is not read
    assert call(t=i32(1000000, -1000000, 0, 0, 0, 0))[1] == "maxt: no context"
    rc, text = call(t=i32(4, 4, 4, 4, 4, 4))
    assert rc == ERR_ARG and "constant" in text and "W = 0" in text
    rc, text = call(t=i32(4, 4, 9, 4, 4, 4), used=u8(1, 1, 0, 1, 1, 1))
    assert rc == ERR_ARG and "constant" in text
    for s in (-1, 65536):
        rc, text = call(strata=i32(0, 1, s, 0, 1, 1))
        assert rc == ERR_ARG and "a stratum outside [0, 2^16)" in text
    assert call(strata=i32(0, 1, 65535, 0, 1, 1))[1] == "maxt: no context"
    for f in (0, -5):
        rc, text = call(first=f)
        assert rc == ERR_ARG and "first must be at least 1" in text
    for r in (0, -1, 1025):
        rc, text = call(R=r)
        assert rc == ERR_ARG and "R outside [1, EAGLE_MAXT_RMAX = 1024]" in text
    rc, text = call(first=2 ** 31 - 1, R=2)
    assert rc == ERR_ARG and "first + R above 2^31" in text
    assert call(first=2 ** 31 - 2, R=2)[1] == "maxt: no context"
    for rows in ((0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 4), (0, 1, 2, 3, 4, 6, 0, 1, 2, 3, 4, 5), (0, 1, 2, 3, 4, -1, 0, 1, 2, 3, 4, 5)):
        rc, text = call(perm=i32(*rows))
        assert rc == ERR_ARG and "no permutation" in text
    assert call(perm=i32(5, 4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 5))[1] == "maxt: no context"
    assert call(perm=i32(2, 1, 0, 0, 1, 2), used=u8(1, 0, 1, 0, 1, 0))[1] == "maxt: no context"          # N = 3: rows of 3
    assert call() == (ERR_ARG, "maxt: no context")                           # nothing wrong but the context
    # through the wrapper an argument error of the library arrives as EagleError(-3) and opens no device
    import torch
    if not torch.cuda.is_available():
        assert not rcpp_api._ctx
    with pytest.raises(rcpp_api.EagleError) as e:
        rcpp_api.maxt(str(tmp_path / "nothing"), (6, 4), [3, 3, 3, 3, 3, 3], R=5)
    assert e.value.code == ERR_ARG and "constant" in e.value.text
    with pytest.raises(rcpp_api.EagleError) as e:
        rcpp_api.maxt(str(tmp_path / "nothing"), (6, 4), [0, 1, 0, 1, 0, 2000000], R=5)
    assert e.value.code == ERR_ARG and "EAGLE_MAXT_TMAX" in e.value.text
