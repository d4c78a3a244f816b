"""CPU: the C ABI of the epistasis scan without a device -- eagle_epistasis_loci and eagle_epistasis_pairs are declared, exported and
bound, section 1b''''ii of the header states the rule and what is not claimed, and every argument error is decided before a context is
needed (ctx == NULL: the text comes through eagle_open_error).  The HIP-free pieces behind them (csrc/eagle_host.h: epi_arg_error,
epi_digits, epi_t53, epi_stat, ...) also run in a stand-alone program under ASan + UBSan, built as tests/test_ibd_abi.py builds its
source, and its integers and bits are compared with Python-int results.  No device work."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import epistasis_truth as truth

ERR_ARG = -3
NAMES = ("eagle_epistasis_loci", "eagle_epistasis_pairs")


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_epistasis_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    assert len(_lib.SIGNATURES["eagle_epistasis_loci"][1]) == 9 and len(_lib.SIGNATURES["eagle_epistasis_pairs"][1]) == 15
    assert re.search(r"#define EAGLE_EPI_MAX_N 65535L", txt) and rcpp_api.EPI_MAX_N == 65535
    assert re.search(r"#define EAGLE_EPI_YMAX 1000000\b", txt) and rcpp_api.EPI_YMAX == 1000000
    assert re.search(r"typedef struct eagle_epi_max \{\s*int64_t i, j;\s*double stat;\s*\}", txt) and C.sizeof(rcpp_api.EpiMax) == 24
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_epi.hip" in makefile and "eagle_epi.o" in makefile
    kern = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_epi.hip")).read()
    code = re.sub(r"//.*", "", kern)
    assert "k_epi_tile" in kern and "k_epi_marker" in kern and "__builtin_amdgcn_mfma_i32_32x32x32_i8" in code and "asm" not in code
    assert "atomicAdd(&sCnt" in code and code.count("atomic") == 1          # the one LDS slot counter; nothing global
    host = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_host.h")).read()
    for piece in ("epi_arg_error", "epi_digits", "epi_t53", "epi_stat", "__ddiv_rn", "__dmul_rn", "__dadd_rn"):
        assert piece in host, piece


def test_header_states_the_rule_and_what_is_not_claimed():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b''''ii."):txt.index("1c.")]
    for phrase in ("y = b0 + b1 g_i + b2 g_j + b3 g_i g_j + e", "additive x additive test of PLINK --epistasis", "F(1, n - 4) of b3 = 0",
                   "a missing call of the source is a heterozygote", "|y_k| <= EAGLE_EPI_YMAX = 1000000", "n <= EAGLE_EPI_MAX_N = 65535",
                   "Y = sum y, T = sum y^2", "s = sum g, q = sum g^2, u = sum y g", "d = sum g_i g_j, e = sum g_i^2 g_j, f = sum g_i g_j^2",
                   "h = sum g_i^2 g_j^2, z = sum y g_i g_j", "balanced digits in [-64, 63]",
                   "B = [[n, s_i, s_j], [s_i, q_i, d], [s_j, d, q_j]], Delta = det B, A = adj B, c = (d, e, f), u = (Y, u_i, u_j)",
                   "Sxx = Delta h - c^T A c", "Sxy = Delta z - c^T A u", "Syy = Delta T - u^T A u", "no term exceeds 2^110",
                   "UNDEFINED (stat = NaN) unless n > 4, Delta > 0 and Sxx > 0", "truncated toward zero to its top 53 bits",
                   "r2 = (t53(Sxy) / t53(Sxx)) (t53(Sxy) / t53(Syy))", "stat = ((double)(n - 4) r2) / (1.0 - r2)", "stat = +inf when !(r2 < 1.0)",
                   "A zero Syy", "lands in +inf, not in NaN", "A hit is stat >= min_stat", "NaN is never a hit",
                   "Agreement with the PLINK or GLIDE programs is neither claimed nor tested", "because neither is available",
                   "Sex chromosomes, dominance terms and case/control traits are out of scope", "1 <= nloci <= 64", "(d, e, f, h, z)",
                   "j - i <= gap on the same chromosome", "ties to the smallest (i, j)", "(-1, -1, NaN)", "always the total number of hits",
                   "untouched otherwise", "returns EAGLE_OK either way", "without global atomics", "prune or filter first",
                   "a multi-device context works on its first device", "decided before the context is used"):
        assert phrase in sec, phrase
    assert txt.index("1b''''i.") < txt.index("1b''''ii.") < txt.index("1c.")
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "Epistasis" in readme and "PLINK or GLIDE programs is neither claimed nor tested" in readme


def test_epistasis_interface_is_public():
    from eagleeverything_amd import am, r_api, rcpp_api
    for name in ("quantise_trait", "epistasis_host", "epistasis_effects", "Epistasis", "EpistasisOfLoci"):
        assert callable(getattr(r_api, name))
    p = inspect.signature(r_api.Epistasis).parameters
    assert [(k, p[k].default) for k in list(p)[2:8]] == [("loci", None), ("map", None), ("gap", 0), ("min_stat", None), ("p", 1e-8),
                                                         ("hit_cap", 1 << 20)]
    assert list(inspect.signature(r_api.epistasis_host).parameters) == ["G", "yq", "loci", "chrom", "gap", "min_stat", "hit_cap"]
    assert list(inspect.signature(am.EpistasisOfLoci).parameters)[:4] == ["AMobj", "trait", "X", "geno"]
    assert list(inspect.signature(rcpp_api.epistasis_loci).parameters)[:4] == ["f_name_ascii_Mt", "dims", "y", "loci"]
    assert list(inspect.signature(rcpp_api.epistasis_pairs).parameters)[:7] == ["f_name_ascii_Mt", "dims", "y", "chrom", "gap", "min_stat", "hit_cap"]
    doc = " ".join(r_api.Epistasis.__doc__.split()) + " ".join(r_api.quantise_trait.__doc__.split())
    for phrase in ("am.reshape_geno(geno, indxNA, view=True)", "half a unit in 10^6", "invariant to a shift and a scale", "fdtri(1, n - 4, 1 - p)"):
        assert phrase in doc, phrase


def test_python_wrappers_refuse_before_the_library(tmp_path):
    import pytest
    from eagleeverything_amd import r_api, rcpp_api
    Mt = str(tmp_path / "Mt.ascii")
    y = np.arange(6)
    for kw in (dict(y=np.arange(5)), dict(y=np.arange(6.0)), dict(y=np.array([0, 0, 0, 0, 0, 1000001]))):
        with pytest.raises(ValueError):
            rcpp_api.epistasis_loci(Mt, (6, 4), kw["y"], [0])
        with pytest.raises(ValueError):
            rcpp_api.epistasis_pairs(Mt, (6, 4), kw["y"])
    with pytest.raises(ValueError):
        rcpp_api.epistasis_loci(Mt, (6, 4), y, [0.5])
    for kw in (dict(chrom=[1, 1, 2]), dict(chrom=[1, 1.5, 2, 2]), dict(gap=-1), dict(min_stat=math.nan), dict(hit_cap=-1)):
        with pytest.raises(ValueError):
            rcpp_api.epistasis_pairs(Mt, (6, 4), y, **kw)
    geno = {"asciifileM": str(tmp_path / "M.ascii"), "asciifileMt": Mt, "dim_of_ascii_M": [6, 4]}
    with pytest.raises(ValueError, match="reshape_geno"):
        r_api.Epistasis(geno, [1.0, 2.0, np.nan, 4.0, 5.0, 6.0], loci=[0])
    with pytest.raises(ValueError, match="constant"):
        r_api.Epistasis(geno, np.full(6, 2.5), loci=[0])
    with pytest.raises(ValueError):
        r_api.Epistasis(geno, np.arange(5.0), loci=[0])


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib, rcpp_api
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()

    n, nm = 6, 9
    i32, i64, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_long)
    dims = (C.c_long * 2)(n, nm)
    y = (C.c_int32 * n)(1, -2, 3, -4, 1000000, -1000000)
    path = str(tmp_path / "Mt.ascii").encode()
    stat, mom = (C.c_double * (nm * 3))(), (C.c_int64 * (nm * 3 * 5))()
    loci = (C.c_long * 3)(0, 8, 8)

    good = (path, dims, y, loci, 3, 8.0, stat, mom)
    names = ("path", "dims", "y", "loci", "nloci", "mem", "stat", "mom")

    def call(**kw):
        return L.eagle_epistasis_loci(None, *[kw.get(k, v) for k, v in zip(names, good)])
    for k in ("path", "dims", "y", "loci", "stat"):
        assert call(**{k: None}) == ERR_ARG and text().startswith("epistasis_loci:") and "NULL" in text(), k
    assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(n, -1)) == ERR_ARG and "dims" in text()
    big = (C.c_int32 * 65536)()
    assert call(dims=(C.c_long * 2)(65536, nm), y=big) == ERR_ARG and "EAGLE_EPI_MAX_N" in text()
    assert call(y=(C.c_int32 * n)(0, 0, 0, 0, 0, 1000001)) == ERR_ARG and "EAGLE_EPI_YMAX" in text()
    assert call(y=(C.c_int32 * n)(-1000001, 0, 0, 0, 0, 0)) == ERR_ARG and "EAGLE_EPI_YMAX" in text()
    assert call(nloci=0) == ERR_ARG and "[1, 64]" in text()
    assert call(loci=(C.c_long * 65)(), nloci=65) == ERR_ARG and "[1, 64]" in text()
    assert call(loci=(C.c_long * 3)(0, 9, 1)) == ERR_ARG and "outside [0, L)" in text()
    assert call(loci=(C.c_long * 3)(0, -1, 1)) == ERR_ARG and "outside [0, L)" in text()
    assert call() == ERR_ARG and "no context" in text()                                  # what passes the rule stops at the missing context
    assert call(mom=None) == ERR_ARG and "no context" in text()
    assert call(dims=(C.c_long * 2)(65535, nm), y=big) == ERR_ARG and "no context" in text()

    cap = 4
    ij, hs, hm = (C.c_int32 * (2 * cap))(), (C.c_double * cap)(), (C.c_int64 * (5 * cap))()
    nh, nt, mx = C.c_long(0), C.c_long(0), rcpp_api.EpiMax()
    chrom = (C.c_int32 * nm)(1, 1, 1, 2, 2, 2, 3, 3, 3)
    good = (path, dims, y, chrom, 2, 10.0, 8.0, ij, hs, hm, cap, C.byref(nh), C.byref(nt), C.byref(mx))
    names = ("path", "dims", "y", "chrom", "gap", "min_stat", "mem", "ij", "hs", "hm", "cap", "nh", "nt", "mx")

    def call(**kw):                                                                       # noqa: F811
        return L.eagle_epistasis_pairs(None, *[kw.get(k, v) for k, v in zip(names, good)])
    for k in ("path", "dims", "y", "nh", "nt", "mx"):
        assert call(**{k: None}) == ERR_ARG and text().startswith("epistasis_pairs:") and "NULL" in text(), k
    assert call(dims=(C.c_long * 2)(n, 0)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(65536, nm), y=big) == ERR_ARG and "EAGLE_EPI_MAX_N" in text()
    assert call(y=(C.c_int32 * n)(0, 0, 0, 1000001, 0, 0)) == ERR_ARG and "EAGLE_EPI_YMAX" in text()
    assert call(gap=-1) == ERR_ARG and "gap" in text()
    assert call(min_stat=math.nan) == ERR_ARG and "NaN" in text()
    assert call(cap=-1) == ERR_ARG and "hit_cap" in text()
    for k in ("ij", "hs", "hm"):
        assert call(**{k: None}) == ERR_ARG and "hit_cap > 0 needs" in text(), k
    assert call() == ERR_ARG and "no context" in text()
    assert call(chrom=None, gap=0, min_stat=-math.inf) == ERR_ARG and "no context" in text()
    assert call(ij=None, hs=None, hm=None, cap=0) == ERR_ARG and "no context" in text()


def py_stat(n, D, Sxx, Sxy, Syy):
    """Rules 4 and 5 on Python ints and floats, written here."""
    if not (n > 4 and D > 0 and Sxx > 0):
        return math.nan

    def t53(x):
        m = abs(x)
        sh = max(0, m.bit_length() - 53)
        v = float((m >> sh) << sh)
        return -v if x < 0 else v
    xy, xx, yy = t53(Sxy), t53(Sxx), t53(Syy)
    if yy == 0.0:
        return math.inf                                         # 0 / 0 = NaN, and !(NaN < 1.0)
    r2 = (xy / xx) * (xy / yy)
    if not r2 < 1.0:
        return math.inf
    return (float(n - 4) * r2) / (1.0 - r2)


def test_epi_host_pieces_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "epi_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_epi_host.cpp"), "-o", exe])
    rng = np.random.default_rng(21)
    cases = []

    def add(G, y, pairs):
        for i, j in pairs:
            t = truth.sums(G[:, i].tolist(), G[:, j].tolist(), y.tolist())
            cases.append(t)
    for n, ymax in ((5, 10), (6, 1000000), (33, 1000), (200, 1000000)):
        G = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(n, 12), p=[0.3, 0.4, 0.3])
        G[:, 3] = G[:, 0]
        G[:, 4] = 1
        y = rng.integers(-ymax, ymax + 1, n)
        add(G, y, [(i, j) for i in range(12) for j in range(i, 12)][:70])
    # the extreme magnitudes: n = 65535, |y| = 10^6 throughout, common alleles (Delta ~ 2^47, Syy's terms ~ 2^107)
    n = 65535
    G = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(n, 4), p=[0.45, 0.1, 0.45])
    G[:, 2] = 1
    G[::2, 2] = -1
    for y in (np.where(rng.random(n) < 0.5, 1000000, -1000000), np.full(n, 1000000), G[:, 0].astype(np.int64) * G[:, 1] * 1000000,
              np.where(G[:, 0] * G[:, 1] > 0, 1000000, -1000000) - (rng.random(n) < 0.01) * 2000000):
        add(G, np.asarray(y, dtype=np.int64), [(0, 1), (1, 0), (0, 2), (2, 3), (1, 1)])
    assert len(cases) >= 300
    keys = ("n", "Y", "T", "si", "qi", "ui", "sj", "qj", "uj", "d", "e", "f", "h", "z")
    inp = tmp_path / "cases.txt"
    inp.write_text("".join(" ".join(str(t[k]) for k in keys) + "\n" for t in cases))
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert "epi host checks passed" in lines[len(cases)]
    kinds = set()
    big = 0
    for t, line in zip(cases, lines):
        w = line.split()
        want = truth.S(t)
        assert tuple(int(x) for x in w[:4]) == want, (t, line)
        big = max(big, max(abs(v) for v in want).bit_length())
        st = np.array([int(w[4], 16)], dtype=np.uint64).view(np.float64)[0]
        ref = py_stat(t["n"], *want)
        if math.isnan(ref):
            assert math.isnan(st)
            kinds.add("nan")
        else:
            assert np.float64(ref).view(np.uint64) == np.float64(st).view(np.uint64), (t, st, ref)
            kinds.add("inf" if math.isinf(ref) else "finite")
    assert kinds == {"nan", "inf", "finite"} and 100 < big <= 110
