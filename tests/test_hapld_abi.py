"""CPU: the C ABI of the pairwise haplotype EM without a device -- eagle_hap_ld is declared, exported and bound, section 1b''''vii of the
header states the rule, the README paragraph states what is and is not claimed, and every argument error is decided before a context
is needed (ctx == NULL: the text comes through eagle_open_error).  No device work."""
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


def test_hap_ld_symbol_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    m = re.search(r"\bint\s+eagle_hap_ld\s*\(([^;]*)\)\s*;", txt)
    assert m, "eagle_hap_ld is not declared in include/eagle_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["eagle_ctx* ctx", "const char* f_name_ascii_Mt", "const long dims[2]", "long window", "double tol", "int max_iter",
                    "double fg_cut", "double dprime_cut", "double max_memory_in_Gbytes", "uint64_t* recomb_mask_out", "uint64_t* strong_mask_out",
                    "double* dprime_out", "double* r2_out", "int64_t* counts_out"]
    assert hasattr(L, "eagle_hap_ld") and hasattr(L, "eagle_dev_hap_ld")
    res, sig = _lib.SIGNATURES["eagle_hap_ld"]
    c_lp, c_dp = C.POINTER(C.c_long), C.POINTER(C.c_double)
    assert res is C.c_int and sig == [C.c_void_p, C.c_char_p, c_lp, C.c_long, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), c_dp, c_dp, C.POINTER(C.c_int64)]
    internal = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_internal.h")).read()
    assert re.search(r"\bint\s+eagle_dev_hap_ld\s*\(\s*eagle_ctx\s*\*", internal)
    mk = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\beagle_hapld\.hip\b", mk, flags=re.M) and re.search(r"^OBJS\s*=.*\beagle_hapld\.o\b", mk, flags=re.M)
    p = inspect.signature(rcpp_api.hap_ld).parameters
    assert list(p)[:2] == ["fMt", "dims"]
    assert (p["window"].default, p["tol"].default, p["max_iter"].default, p["fg_cut"].default, p["dprime_cut"].default, p["bands"].default) == \
        (50, 1e-10, 1000, 0.01, 0.8, False)


def test_header_states_the_rule():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b''''vii."):txt.index("1c.")]
    for phrase in ("a missing call is a het", "Allele B is the allele of '2'", "b_i = n + s_i", "polymorphic iff 0 < b_i < 2n",
                   "d = sum g_i g_j", "e = sum g_i^2 g_j^2", "f = sum g_i^2 g_j", "h = sum g_i g_j^2",
                   "N22 = (e + f + h + d) / 4", "N00 = (e - f - h + d) / 4", "N20 = (e - f + h - d) / 4", "N02 = (e + f - h - d) / 4",
                   "N12 = (q_j + s_j - e - f) / 2", "N10 = (q_j - s_j - e + f) / 2", "N21 = (q_i + s_i - e - h) / 2", "N01 = (q_i - s_i - e + h) / 2",
                   "N11 = x = n - q_i - q_j + e", "k_BB = 2 N22 + N21 + N12", "k_BA = 2 N20 + N21 + N10", "k_AB = 2 N02 + N01 + N12",
                   "k_AA = 2 N00 + N01 + N10", "nothing contracts into an FMA", "T = (double)(2n)", "never as 1 - p_i", "Start at equilibrium",
                   "With x = 0 there is no iteration", "t = den > 0 ? u / den : 0.5", "xo = x - xt", "delta = |pBB_new - pBB|",
                   "stop with code 0 when delta <= tol", "code 1 when iterations = max_iter", "tol = 1e-10 and max_iter = 1000",
                   "Haploview's EM", "not PLINK's cubic solver", "Dmax = min(p_i q_j, q_i p_j) when D >= 0, else min(p_i p_j, q_i q_j)",
                   "clamped to [-1, 1]", "r2_h = (D D) / ((p_i q_i)(p_j q_j))", "iff pmin > fg_cut, strictly", "iff |D'| >= dprime_cut",
                   "D' is reported as -2.0 and r2_h as -1.0", "With n = 1 no pair is defined", "bit o - 1 of row i is the pair (i, i + o)",
                   "Each of the four may be NULL", "the defined pairs, the pairs that stopped with code 1, the recombinant bits, the strong bits",
                   "g.g, g^2.g^2, g^2.g and g.g^2", "neither claimed nor tested", "Gabriel's confidence-interval blocks", "nine products",
                   "a picks mode against listed loci", "multi-marker haplotype frequencies inside a block", "sex chromosomes",
                   "decided before the context is used"):
        assert phrase in sec, phrase
    assert txt.index("1b''''vi.") < txt.index("1b''''vii.") < txt.index("1c.")


def test_readme_and_design_state_the_pass():
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    for phrase in ("r_api.HapLD(geno, window=50, map=None, kb=None)", "r_api.HapBlocks(geno, method=\"fourgamete\"", "sets_from_blocks",
                   "`k_hapld_tile`", "`r_api.hap_ld_host`", "§1b''''vii", "not PLINK's cubic solver", "Gabriel's confidence-interval blocks",
                   "neither claimed nor tested", "tools/hapld_timing.py", "profiles/r25_hapld.json"):
        assert phrase in readme, phrase
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    for phrase in ("### 4.8u", "`k_hapld_tile`", "until the slowest pair of the wave stops", "no scratch", "52,224", "contract(off)"):
        assert phrase in design, phrase


def test_interface_is_public():
    from eagleeverything_amd import r_api
    for name in ("hap_ld_host", "hap_ld_pairs_host", "hap_ld_cells", "hap_blocks_host", "HapLD", "HapBlocks", "sets_from_blocks"):
        assert callable(getattr(r_api, name))
    p = inspect.signature(r_api.HapLD).parameters
    assert list(p)[:4] == ["geno", "window", "map", "kb"] and (p["window"].default, p["map"].default, p["kb"].default) == (50, None, None)
    p = inspect.signature(r_api.HapBlocks).parameters
    assert list(p)[:8] == ["geno", "method", "window", "map", "kb", "min_snp", "fg_cut", "dprime"]
    assert (p["method"].default, p["window"].default, p["min_snp"].default, p["fg_cut"].default, p["dprime"].default) == ("fourgamete", 50, 2, 0.01, 0.8)
    assert list(inspect.signature(r_api.hap_blocks_host).parameters) == ["recomb", "strong", "window", "chrom", "pos", "kb", "method", "min_snp"]
    p = inspect.signature(r_api.sets_from_blocks).parameters
    assert list(p) == ["blocks", "max_markers", "names"] and (p["max_markers"].default, p["names"].default) == (64, None)
    p = inspect.signature(r_api.hap_ld_host).parameters
    assert list(p)[:2] == ["Mt8", "window"] and (p["tol"].default, p["max_iter"].default, p["fg_cut"].default, p["dprime_cut"].default) == (1e-10, 1000, 0.01, 0.8)


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()

    nm, w = 7, 50
    dims = (C.c_long * 2)(5, nm)
    rec, strong = (C.c_uint64 * nm)(), (C.c_uint64 * nm)()
    dp, r2 = (C.c_double * (nm * w))(), (C.c_double * (nm * w))()
    counts = (C.c_int64 * 4)()
    good = (str(tmp_path / "Mt.ascii").encode(), dims, w, 1e-10, 1000, 0.01, 0.8, 8.0, rec, strong, dp, r2, counts)
    names = ("path", "dims", "window", "tol", "max_iter", "fg_cut", "dprime_cut", "mem", "rec", "strong", "dp", "r2", "counts")

    def call(**kw):
        return L.eagle_hap_ld(None, *[kw.get(k, v) for k, v in zip(names, good)])
    assert call(path=None) == ERR_ARG and "hap_ld" in text() and "NULL" in text()
    assert call(dims=None) == ERR_ARG and "NULL" in text()
    assert call(counts=None) == ERR_ARG and "NULL" in text()
    assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims must be positive" in text()
    assert call(dims=(C.c_long * 2)(5, -1)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(1 << 30, nm)) == ERR_ARG and "2^30 individuals or more" in text()
    for bad in (0, 257, -3):
        assert call(window=bad) == ERR_ARG and "window must be in [1, 256]" in text()
    for bad in (0.0, 1.0, -1e-3, float("nan")):
        assert call(tol=bad) == ERR_ARG and "tol must be in (0, 1)" in text()
    for bad in (0, 100001, -1):
        assert call(max_iter=bad) == ERR_ARG and "max_iter must be in [1, 100000]" in text()
    for bad in (-0.01, 1.01, float("nan")):
        assert call(fg_cut=bad) == ERR_ARG and "fg_cut must be in [0, 1]" in text()
        assert call(dprime_cut=bad) == ERR_ARG and "dprime_cut must be in [0, 1]" in text()
    # the limits themselves, and every output but the counts left out, pass the argument checks
    assert call() == ERR_ARG and "no context" in text()
    assert call(dims=(C.c_long * 2)((1 << 30) - 1, nm), window=256, max_iter=100000, fg_cut=0.0, dprime_cut=1.0) == ERR_ARG and "no context" in text()
    assert call(window=1, max_iter=1, fg_cut=1.0, dprime_cut=0.0, tol=0.5) == ERR_ARG and "no context" in text()
    assert call(rec=None, strong=None, dp=None, r2=None) == ERR_ARG and "no context" in text()


def test_python_layer_refuses_bad_arguments(tmp_path):
    from eagleeverything_amd import r_api
    geno = {"asciifileM": str(tmp_path / "M.ascii"), "asciifileMt": str(tmp_path / "Mt.ascii"), "dim_of_ascii_M": (5, 7)}
    bim = {"Chr": ["1"] * 7, "Pos": list(range(7))}
    for fn in (r_api.HapLD, r_api.HapBlocks):
        with pytest.raises(ValueError):
            fn(geno, kb=5)                                                   # kb needs a map
        with pytest.raises(ValueError):
            fn(geno, map={"Chr": ["1"] * 6, "Pos": list(range(6))})          # a map of another panel
        with pytest.raises(ValueError):
            fn(geno, map=bim, kb=0.0001)
        with pytest.raises(ValueError):
            fn(geno, map={"Chr": ["1"] * 7, "Pos": [0.5] * 7})
    none = np.zeros((7, 1), dtype=np.uint64)
    for kw in (dict(window=0), dict(window=257), dict(min_snp=0)):
        with pytest.raises(ValueError):
            r_api.hap_blocks_host(none, none, **{"window": 4, **kw})
