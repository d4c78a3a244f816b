"""CPU: the C ABI of the transmission disequilibrium test without a device -- eagle_tdt and eagle_bed_tdt are declared, exported and bound,
section 1b''''viii of the header states the rule and what is not claimed, and every argument error of rules 5 and 6 is decided before a
context is needed (ctx == NULL: the text comes through eagle_open_error).  The HIP-free pieces behind them (csrc/eagle_host.h: tdt_words,
tdt_sign, tdt_families, tdt_arg_error) also run in a stand-alone program under ASan + UBSan, built as tests/test_mendel_abi.py builds
its source.  No device work."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
NAMES = ("eagle_tdt", "eagle_bed_tdt")


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_tdt_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    assert [len(_lib.SIGNATURES[name][1]) for name in NAMES] == [16, 17]
    assert rcpp_api.TDT_MAX_FLIP_TRIOS == 65535 == rcpp_api.MAXT_MAX_N
    ctxh = read("eagleeverything_amd", "csrc", "eagle_ctx.h")
    for name in ("eagle_dev_tdt_trios", "eagle_dev_tdt_finish", "eagle_dev_tdt_image", "eagle_dev_tdt_signs"):
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, ctxh) and hasattr(L, name)
    makefile = read("eagleeverything_amd", "csrc", "Makefile")
    assert "eagle_tdt.hip" in makefile and "eagle_tdt.o" in makefile
    kern = read("eagleeverything_amd", "csrc", "eagle_tdt.hip")
    for k in ("k_tdt_trios", "k_tdt_finish", "k_tdt_image", "k_tdt_signs", "tdt_words(", "tdt_sign(", "__ddiv_rn(__dmul_rn("):
        assert k in kern
    assert "asm" not in re.sub(r"//.*", "", kern)
    # both entry points run through one function that calls the one plane builder with the route's name as a variable, and the flips'
    # product is the max(T) tile as it stands
    ing = read("eagleeverything_amd", "csrc", "eagle_ingest.cpp")
    assert len(re.findall(r"\bg\.build\(ctx, who,", ing)) == 1 and len(re.findall(r"\btdt_call\(ctx, \"", ing)) == 2
    flat = " ".join(ing.split())
    assert "eagle_dev_maxt_tile(ctx, 0, img.as<int8_t>(), rows, ntrios, plan.ld, op.as<int8_t>(), plan.ld, 1, R, R, 1, 0," in flat
    assert "eagle_dev_maxt_finish(ctx, pkey.as<double>(), parg.as<int32_t>(), tile_base, R," in flat
    assert "k_tdt_tile" not in kern and "mfma" not in kern


def test_header_states_the_rule_and_what_is_not_claimed():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b''''viii."):txt.index("1c.")]
    for phrase in ("Spielman 1993", "K = C_c & C_f & C_m & ~E", "Hf = H_f & K and Hm = H_m & K", "A trio with an unknown parent is legal and contributes nothing",
                   "A2 is the allele of genotype +1", "PT = Hf & (B_c | H_c & A_m)", "PU = Hf & (A_c | H_c & B_m)", "MT = Hm & (B_c | H_c & A_f)",
                   "MU = Hm & (A_c | H_c & B_f)", "W = Hf & Hm & H_c", "11 are informative", "d = PT + MT - PU - MU lies in [-2, 2]",
                   "L x 5 int32 = (PT, PU, MT, MU, W)", "a trio listed twice counts twice", "T = PT + MT + W, U = PU + MU + W, d_obs = T - U, V = T + U",
                   "key_obs = fl(fl(d d) / V)", "0 where V = 0", "(popcount K, popcount Hf, popcount Hm, T_t, U_t, W_t)", "For R >= 1 only",
                   "int32 in [0, 65535]", "the smallest list position k with (f_k, m_k) = (f_t, m_t)", "full sibs flip together",
                   "the sign -1 when bit 31 of h is set, else +1", "counter = r 2^16 + phi + 1", "V does not change under a flip",
                   "#{r : |d_m^(r)| >= |d_obs,m|}, compared as integers", "the lowest marker that attains it", "add and concatenate exactly as eagle_maxt's do",
                   "ntrios in [1, 2^27] when R = 0", "ntrios <= 65,535, R <= 1024 per call and first + R <= 2^31 when R >= 1", "panel markers < 2^31",
                   "bands of whole 128-marker tiles", "EAGLE_ERR_NOMEM, decided before any kernel runs", "decided before the context is used",
                   "Agreement with the PLINK program is neither claimed nor tested", "Every marker is autosomal",
                   "a missing call is a het, which invents informative parents", "Sib-TDT / DFAM, parental discordance tests, adaptive permutation, "
                   "covariates and several devices are out of scope"):
        assert phrase in sec, phrase
    assert txt.index("1b''''vii.") < txt.index("1b''''viii.") < txt.index("1c.")
    readme = " ".join(read("README.md").split())
    assert "Transmission disequilibrium test" in readme and "r_api.TDT" in readme
    design = read("DESIGN.md")
    assert "4.8v" in design and "k_tdt_trios" in design


def test_tdt_interface_is_public():
    from eagleeverything_amd import r_api, rcpp_api
    import eagleeverything_amd
    for name in ("tdt_host", "tdt_families", "tdt_signs_host", "tdt_summary", "tdt_merge", "TDT"):
        assert callable(getattr(r_api, name))
    p = inspect.signature(r_api.TDT).parameters
    assert [(k, p[k].default) for k in list(p)[1:]] == [("trios", None), ("fam", None), ("affected", None), ("bed", None), ("include", None), ("map", None),
                                                        ("R", 0), ("seed", 0), ("family", None), ("first", 1), ("availmemGb", 8), ("device", 0)]
    p = inspect.signature(r_api.tdt_host).parameters
    assert [(k, p[k].default) for k in list(p)[3:]] == [("family", None), ("seed", 0), ("first", 1), ("R", 0)] and list(p)[:3] == ["g", "called", "trios"]
    assert list(inspect.signature(rcpp_api.tdt).parameters)[:7] == ["f_name_ascii_M", "dims", "trios", "family", "seed", "first", "R"]
    assert list(inspect.signature(rcpp_api.bed_tdt).parameters)[:8] == ["bed_path", "dims", "trios", "include", "family", "seed", "first", "R"]
    doc = " ".join(r_api.TDT.__doc__.split()) + " ".join(r_api.tdt_summary.__doc__.split())
    for phrase in ("agreement with that program is not claimed", "every marker is taken as autosomal", "route for un-imputed panels",
                   "immune to population stratification", "z_poo", "(p1 - p2) / sqrt(p (1 - p) (1 / n1 + 1 / n2))", "no other program's"):
        assert phrase in doc, phrase
    assert "TDT" in eagleeverything_amd.__doc__


def i32(*v):
    return (C.c_int32 * len(v))(*v)


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()

    nm, n = 7, 5
    dims = (C.c_long * 2)(n, nm)
    tab, mk, key = (C.c_int32 * (6 * 4))(), (C.c_int32 * (5 * nm))(), (C.c_double * nm)()
    c1, mx, am = (C.c_int32 * nm)(), (C.c_double * 4)(), (C.c_int32 * 4)()
    trios = i32(2, 0, 1, 2, 0, 1, 3, -1, 1, 4, -1, -1)
    fam = i32(0, 0, 65535, 3)
    for fn, who, good, names in (
            (L.eagle_tdt, "tdt", (str(tmp_path / "M.ascii").encode(), dims, trios, 4, fam, 9, 1, 4, 8.0, tab, mk, key, c1, mx, am),
             ("path", "dims", "trios", "ntrios", "family", "seed", "first", "R", "mem", "tab", "mk", "key", "c1", "mx", "am")),
            (L.eagle_bed_tdt, "bed_tdt", (str(tmp_path / "p.bed").encode(), dims, None, trios, 4, fam, 9, 1, 4, 8.0, tab, mk, key, c1, mx, am),
             ("path", "dims", "include", "trios", "ntrios", "family", "seed", "first", "R", "mem", "tab", "mk", "key", "c1", "mx", "am"))):

        def call(**kw):
            return fn(None, *[kw.get(k, v) for k, v in zip(names, good)])
        for k in ("path", "dims", "trios", "tab", "mk", "key"):
            assert call(**{k: None}) == ERR_ARG and text().startswith(who + ":") and "NULL" in text(), k
        for k in ("c1", "mx", "am"):                     # needed with flips only
            assert call(**{k: None}) == ERR_ARG and "NULL" in text(), k
            assert call(**{k: None, "R": 0}) == ERR_ARG and "no context" in text(), k
        assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
        assert call(dims=(C.c_long * 2)(n, -1)) == ERR_ARG and "dims" in text()
        assert call(dims=(C.c_long * 2)(n, 1 << 31)) == ERR_ARG and "2^31" in text()
        assert call(ntrios=0) == ERR_ARG and "number of trios" in text() and text().startswith(who + ":")
        assert call(ntrios=(1 << 27) + 1, R=0) == ERR_ARG and "number of trios" in text()
        assert call(ntrios=65536) == ERR_ARG and "65535 trios" in text()
        assert call(R=-1) == ERR_ARG and "negative" in text()
        assert call(R=1025) == ERR_ARG and "1024" in text()
        assert call(first=0) == ERR_ARG and "first must be at least 1" in text()
        assert call(first=(1 << 31) - 3) == ERR_ARG and "above 2^31" in text()
        assert call(family=i32(0, 0, 65536, 3)) == ERR_ARG and "family" in text()
        assert call(family=i32(0, -1, 0, 3)) == ERR_ARG and "family" in text()
        for bad, k in ((i32(2, 0, 1, 2, 2, 1), 1), (i32(2, 0, 2, 2, 0, 1), 0), (i32(2, 0, 1, 3, 1, 1), 1), (i32(2, 0, 1, 5, 0, 1), 1),
                       (i32(-1, 0, 1, 2, 0, 1), 0), (i32(2, 5, 1, 2, 0, 1), 0), (i32(2, 0, 1, 2, 0, -2), 1)):
            assert call(trios=bad, ntrios=2, family=None) == ERR_ARG and "trio %d is not (c, f, m)" % k in text(), list(bad)
        # what passes the rule stops at the missing context: no families, counts only (first and the families are then not read), the limits
        assert call() == ERR_ARG and "no context" in text()
        assert call(family=None) == ERR_ARG and "no context" in text()
        assert call(R=0, first=0, family=i32(-1, -1, -1, -1)) == ERR_ARG and "no context" in text()
        assert call(first=(1 << 31) - 4) == ERR_ARG and "no context" in text()
        assert call(dims=(C.c_long * 2)(n, (1 << 31) - 1)) == ERR_ARG and "no context" in text()

    # the .bed entry point's own
    inc0 = (C.c_uint8 * nm)()
    bed = str(tmp_path / "p.bed").encode()
    rest = (trios, 4, fam, 9, 1, 4, 8.0, tab, mk, key, c1, mx, am)
    assert L.eagle_bed_tdt(None, bed, (C.c_long * 2)(1 << 30, nm), None, *rest) == ERR_ARG and "2^30" in text()
    assert L.eagle_bed_tdt(None, bed, dims, inc0, *rest) == ERR_ARG and "no marker" in text()


def test_python_wrappers_refuse_before_the_library(tmp_path, monkeypatch):
    from eagleeverything_amd import _lib, rcpp_api

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    M, bed = str(tmp_path / "M.ascii"), str(tmp_path / "a.bed")
    for trios in ([], [[0, 1]], [0, 1, 2], [[0, 0, 1]], [[0, 1, 0]], [[0, 1, 1]], [[4, 0, 1]], [[0, 4, 1]], [[0, 1, -2]], [[0, 1.5, 2]], [[-1, 0, 1]]):
        with pytest.raises(ValueError):
            rcpp_api.tdt(M, (4, 6), trios)
        with pytest.raises(ValueError):
            rcpp_api.bed_tdt(bed, (4, 6), trios)
    for kw in (dict(R=-1), dict(R=2.5), dict(R=1, first=0), dict(R=2, first=(1 << 31) - 1), dict(R=1, family=[0, 1]), dict(R=1, family=[65536]),
               dict(R=1, family=[-1]), dict(R=1, family=[[0]]), dict(R=1, family=[0.5]), dict(seed=0.5), dict(R=1, first=1.5)):
        with pytest.raises(ValueError):
            rcpp_api.tdt(M, (4, 6), [[2, 0, 1]], **kw)
        with pytest.raises(ValueError):
            rcpp_api.bed_tdt(bed, (4, 6), [[2, 0, 1]], **kw)
    with pytest.raises(ValueError):
        rcpp_api.bed_tdt(bed, (4, 6), [[0, 1, 2]], include=[1, 0, 1])
    with pytest.raises(ValueError):
        rcpp_api.tdt(M, (4, 1 << 31), [[0, 1, 2]])
    with pytest.raises(ValueError):
        rcpp_api.tdt(M, (70000, 6), np.stack([np.arange(2, 65538), np.zeros(65536), np.ones(65536)], axis=1), R=1)
    with pytest.raises(AssertionError):                  # what passes the checks reaches the library
        rcpp_api.tdt(M, (4, 6), [[2, 0, 1]], family=[65535], seed=-1, first=(1 << 31) - 1, R=1)
    tr, fam, seed, first, R = rcpp_api.tdt_args("t", [[2, 0, 1], [3, -1, 1]], 4, 6, [7, 7], -1, 5, 3)
    assert tr.dtype == np.int32 and fam.dtype == np.int32 and fam.tolist() == [7, 7] and (seed, first, R) == (2 ** 64 - 1, 5, 3)
    assert rcpp_api.tdt_args("t", [[2, 0, 1]], 4, 6, [99999], 0, 0, 0)[1] is None          # R = 0: the families are not read


def test_tdt_host_pieces_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "tdt_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_tdt_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tdt host checks passed" in r.stdout
