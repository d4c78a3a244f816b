"""CPU: the C ABI of the Mendel errors and the parentage assignment without a device -- eagle_mendel, eagle_bed_mendel, eagle_parentage and
eagle_bed_parentage are declared, exported and bound, section 1b'''viii of the header states the rule and what is not claimed, and every
argument error of rules 2, 6 and 7 is decided before a context is needed (ctx == NULL: the text comes through eagle_open_error).  The
HIP-free pieces behind them (csrc/eagle_host.h: mendel_error_word, mendel_trios_check, parentage_arg_error, parentage_list_check, ...)
also run in a stand-alone program under ASan + UBSan, built as tests/test_ibd_abi.py builds its source.  No device work."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
NAMES = ("eagle_mendel", "eagle_bed_mendel", "eagle_parentage", "eagle_bed_parentage")


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_mendel_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    assert [len(_lib.SIGNATURES[name][1]) for name in NAMES] == [8, 9, 13, 14]
    assert re.search(r"#define EAGLE_MENDEL_MAX_TRIOS 134217728L", txt) and rcpp_api.MENDEL_MAX_TRIOS == 134217728
    ctxh = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ctx.h")).read()
    for name in ("eagle_dev_mendel_trios", "eagle_dev_plane_gather", "eagle_dev_parentage"):
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, ctxh) and hasattr(L, name)
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_mendel.hip" in makefile and "eagle_mendel.o" in makefile
    kern = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_mendel.hip")).read()
    for k in ("k_mendel_trios", "k_plane_gather", "k_parentage", "k_parentage_finish"):
        assert k in kern
    assert "asm" not in re.sub(r"//.*", "", kern)
    # one helper builds the planes of all six entry points: one launch site per source (the image through the line walker, the .bed ring)
    ing = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ingest.cpp")).read()
    assert len(re.findall(r"\bg\.build\(ctx, \"", ing)) == 6
    assert len(re.findall(r"eagle_dev_ibd_planes_i8\(", ing)) == 1 and len(re.findall(r"eagle_dev_ibd_planes_bed\(", ing)) == 1


def test_header_states_the_rule_and_what_is_not_claimed():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b'''viii."):txt.index("1b''''.")]
    for phrase in ("Agreement with the PLINK program is neither claimed nor tested", "every marker is autosomal",
                   "Setting erroneous genotypes to missing is out of scope", "code 01 is not called", "a missing call of the original data is a het",
                   "A parent index -1 is an unknown parent and behaves as an individual that is called nowhere",
                   "a trio with both parents -1 is legal and has no errors", "c != f, c != m",
                   "no choice of one allele from each parent gives the child's genotype", "can pass either allele", "exactly 16 are errors",
                   "H_c = C_c & ~A_c & ~B_c", "X = A_c B_f | B_c A_f", "U = A_c | H_c B_f", "V = B_c | H_c A_f", "E = X | U B_m | V A_m",
                   "past the last marker are masked", "(n_cf, e_cf, n_cm, e_cm, n_trio, e)", "n_ = L for known parents and 0 otherwise",
                   "PLINK's .lmendel", "any order gives the same result", "a duplicate inside a list is EAGLE_ERR_ARG", "one unknown dam",
                   "both empty is EAGLE_ERR_ARG", "s != c, d != c, overlap >= min_overlap, and s != d unless allow_self",
                   "for single-parent assignment it is n_cf", "ordinal = s_idx max(n_d, 1) + d_idx", "the smaller key wins",
                   "THE RANK IS BY ERROR COUNT, NOT BY ERROR RATE", "(sire, dam, e, overlap)", "all four are -1 where there is no such candidate",
                   "EAGLE_MENDEL_MAX_TRIOS = 2^27", "max(n_s, 1) max(n_d, 1) < 2^31", "panel markers < 2^31",
                   "EAGLE_ERR_NOMEM, decided before any kernel runs", "Single device", "decided before the context is used"):
        assert phrase in sec, phrase
    assert txt.index("1b'''vii.") < txt.index("1b'''viii.") < txt.index("1b''''.")
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "Mendel errors and parentage" in readme and "Agreement with the PLINK program is neither claimed nor tested" in readme
    assert "by error count, not by rate" in readme


def test_mendel_interface_is_public():
    from eagleeverything_amd import r_api, rcpp_api
    for name in ("ReadFam", "fam_trios", "mendel_host", "parentage_host", "Mendel", "mendel_keep_mask", "Parentage"):
        assert callable(getattr(r_api, name))
    p = inspect.signature(r_api.Mendel).parameters
    assert [(k, p[k].default) for k in list(p)[1:7]] == [("trios", None), ("fam", None), ("bed", None), ("include", None), ("map", None),
                                                         ("availmemGb", 8)]
    p = inspect.signature(r_api.Parentage).parameters
    assert [(k, p[k].default) for k in list(p)[2:9]] == [("sires", None), ("dams", None), ("bed", None), ("include", None), ("min_overlap", 1),
                                                         ("allow_self", False), ("max_rate", 0.01)]
    assert list(inspect.signature(r_api.mendel_host).parameters) == ["g", "called", "trios"]
    assert list(inspect.signature(r_api.parentage_host).parameters) == ["g", "called", "offspring", "sires", "dams", "min_overlap", "allow_self"]
    assert list(inspect.signature(r_api.mendel_keep_mask).parameters) == ["marker_err", "ntrios", "max_rate"]
    assert list(inspect.signature(rcpp_api.mendel).parameters)[:3] == ["f_name_ascii_M", "dims", "trios"]
    assert list(inspect.signature(rcpp_api.bed_mendel).parameters)[:4] == ["bed_path", "dims", "trios", "include"]
    assert list(inspect.signature(rcpp_api.parentage).parameters)[:7] == ["f_name_ascii_M", "dims", "offspring", "sires", "dams", "min_overlap",
                                                                          "allow_self"]
    assert list(inspect.signature(rcpp_api.bed_parentage).parameters)[:8] == ["bed_path", "dims", "offspring", "sires", "dams", "include",
                                                                              "min_overlap", "allow_self"]
    doc = " ".join(r_api.Parentage.__doc__.split()) + " ".join(r_api.Mendel.__doc__.split())
    for phrase in ("THE RANK IS BY ERROR COUNT, NOT BY RATE", "agreement with that program is not claimed", "every marker is taken as autosomal",
                   "route for un-imputed panels"):
        assert phrase in doc, phrase


def i32(*v):
    return (C.c_int32 * len(v))(*v)


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()

    nm, n = 7, 5
    dims = (C.c_long * 2)(n, nm)
    tab, mk, best = (C.c_int32 * (6 * 8))(), (C.c_int32 * nm)(), (C.c_int32 * (8 * 4))()
    trios = i32(2, 0, 1, 2, 0, 1, 3, -1, 1, 4, -1, -1)
    for fn, who, good, names in (
            (L.eagle_mendel, "mendel", (str(tmp_path / "M.ascii").encode(), dims, trios, 4, 8.0, tab, mk),
             ("path", "dims", "trios", "ntrios", "mem", "tab", "mk")),
            (L.eagle_bed_mendel, "bed_mendel", (str(tmp_path / "p.bed").encode(), dims, None, trios, 4, 8.0, tab, mk),
             ("path", "dims", "include", "trios", "ntrios", "mem", "tab", "mk"))):

        def call(**kw):
            return fn(None, *[kw.get(k, v) for k, v in zip(names, good)])
        assert call(path=None) == ERR_ARG and text().startswith(who + ":") and "NULL" in text()
        assert call(dims=None) == ERR_ARG and "NULL" in text()
        assert call(trios=None) == ERR_ARG and "NULL" in text()
        assert call(tab=None) == ERR_ARG and "NULL" in text()
        assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
        assert call(dims=(C.c_long * 2)(n, -1)) == ERR_ARG and "dims" in text()
        assert call(dims=(C.c_long * 2)(n, 1 << 31)) == ERR_ARG and "2^31" in text()
        assert call(ntrios=0) == ERR_ARG and "number of trios" in text() and text().startswith(who + ":")
        assert call(ntrios=-1) == ERR_ARG and "number of trios" in text()
        assert call(ntrios=(1 << 27) + 1) == ERR_ARG and "number of trios" in text()
        for bad, k in ((i32(2, 0, 1, 2, 2, 1), 1), (i32(2, 0, 2, 2, 0, 1), 0), (i32(2, 0, 1, 3, 1, 1), 1), (i32(2, 0, 1, 5, 0, 1), 1),
                       (i32(-1, 0, 1, 2, 0, 1), 0), (i32(2, 5, 1, 2, 0, 1), 0), (i32(2, 0, 1, 2, 0, -2), 1), (i32(2, 0, 1, 2, -2, 0), 1)):
            assert call(trios=bad, ntrios=2) == ERR_ARG and "trio %d is not (c, f, m)" % k in text(), list(bad)
        # what passes the rule stops at the missing context: repeats, unknown parents, both unknown, no marker counts
        assert call() == ERR_ARG and "no context" in text()
        assert call(mk=None) == ERR_ARG and "no context" in text()
        assert call(dims=(C.c_long * 2)(n, (1 << 31) - 1)) == ERR_ARG and "no context" in text()

    off, sires, dams = i32(2, 3), i32(0, 1, 4), i32(1, 0, 2)
    for fn, who, good, names in (
            (L.eagle_parentage, "parentage", (str(tmp_path / "M.ascii").encode(), dims, off, 2, sires, 3, dams, 3, 1, 0, 8.0, best),
             ("path", "dims", "off", "n_o", "sires", "n_s", "dams", "n_d", "min_overlap", "allow_self", "mem", "best")),
            (L.eagle_bed_parentage, "bed_parentage", (str(tmp_path / "p.bed").encode(), dims, None, off, 2, sires, 3, dams, 3, 1, 0, 8.0, best),
             ("path", "dims", "include", "off", "n_o", "sires", "n_s", "dams", "n_d", "min_overlap", "allow_self", "mem", "best"))):

        def call(**kw):
            return fn(None, *[kw.get(k, v) for k, v in zip(names, good)])
        assert call(path=None) == ERR_ARG and text().startswith(who + ":") and "NULL" in text()
        assert call(dims=None) == ERR_ARG and "NULL" in text()
        assert call(off=None) == ERR_ARG and "NULL" in text()
        assert call(best=None) == ERR_ARG and "NULL" in text()
        assert call(sires=None) == ERR_ARG and "NULL" in text()                        # a positive length needs the list
        assert call(dams=None) == ERR_ARG and "NULL" in text()
        assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
        assert call(dims=(C.c_long * 2)(n, 1 << 31)) == ERR_ARG and "2^31 markers" in text()
        assert call(n_o=0) == ERR_ARG and "number of offspring" in text() and text().startswith(who + ":")
        assert call(n_o=(1 << 27) + 1) == ERR_ARG and "number of offspring" in text()
        assert call(n_s=0, n_d=0) == ERR_ARG and "both candidate lists are empty" in text()
        assert call(n_s=-1) == ERR_ARG and "negative length" in text()
        assert call(n_s=1 << 16, n_d=1 << 15) == ERR_ARG and "below 2^31" in text()
        assert call(min_overlap=-1) == ERR_ARG and "min_overlap" in text()
        assert call(min_overlap=1 << 31) == ERR_ARG and "min_overlap" in text()
        assert call(allow_self=2) == ERR_ARG and "allow_self" in text()
        assert call(off=i32(2, 2)) == ERR_ARG and "offspring entry 1 is a duplicate" in text()
        assert call(sires=i32(0, 1, 0)) == ERR_ARG and "sires entry 2 is a duplicate" in text()
        assert call(dams=i32(2, 0, 2)) == ERR_ARG and "dams entry 2 is a duplicate" in text()
        assert call(off=i32(2, 5)) == ERR_ARG and "offspring entry 1 is outside [0, n)" in text()
        assert call(sires=i32(-1, 1, 4)) == ERR_ARG and "sires entry 0 is outside" in text()
        assert call(dams=i32(1, 0, 5)) == ERR_ARG and "dams entry 2 is outside" in text()
        # what passes: an individual in several lists, the offspring among the candidates, one empty list, selfing, min_overlap 0
        assert call() == ERR_ARG and "no context" in text()
        assert call(sires=i32(2, 3, 0), dams=i32(2, 3, 0), allow_self=1, min_overlap=0) == ERR_ARG and "no context" in text()
        assert call(dams=None, n_d=0) == ERR_ARG and "no context" in text()
        assert call(sires=None, n_s=0) == ERR_ARG and "no context" in text()

    # the .bed entry points' own
    inc0 = (C.c_uint8 * nm)()
    bed = str(tmp_path / "p.bed").encode()
    assert L.eagle_bed_mendel(None, bed, (C.c_long * 2)(1 << 30, nm), None, trios, 4, 8.0, tab, mk) == ERR_ARG and "2^30" in text()
    assert L.eagle_bed_mendel(None, bed, dims, inc0, trios, 4, 8.0, tab, mk) == ERR_ARG and "no marker" in text()
    assert L.eagle_bed_parentage(None, bed, (C.c_long * 2)(1 << 30, nm), None, off, 2, sires, 3, dams, 3, 1, 0, 8.0, best) == ERR_ARG and "2^30" in text()
    assert L.eagle_bed_parentage(None, bed, dims, inc0, off, 2, sires, 3, dams, 3, 1, 0, 8.0, best) == ERR_ARG and "no marker" in text()


def test_python_wrappers_refuse_before_the_library(tmp_path):
    from eagleeverything_amd import rcpp_api
    M, bed = str(tmp_path / "M.ascii"), str(tmp_path / "a.bed")
    for trios in ([], [[0, 1]], [0, 1, 2], [[0, 0, 1]], [[0, 1, 0]], [[0, 1, 1]], [[4, 0, 1]], [[0, 4, 1]], [[0, 1, -2]], [[0, 1.5, 2]], [[-1, 0, 1]]):
        with pytest.raises(ValueError):
            rcpp_api.mendel(M, (4, 6), trios)
        with pytest.raises(ValueError):
            rcpp_api.bed_mendel(bed, (4, 6), trios)
    with pytest.raises(ValueError):
        rcpp_api.bed_mendel(bed, (4, 6), [[0, 1, 2]], include=[1, 0, 1])
    for kw in (dict(offspring=[]), dict(offspring=[0, 0]), dict(offspring=[4]), dict(offspring=[0.5]), dict(sires=[1, 1]), dict(dams=[2, 2]),
               dict(sires=[-1]), dict(dams=[4]), dict(sires=None, dams=None), dict(sires=[], dams=[]), dict(min_overlap=-1), dict(min_overlap=1.5),
               dict(min_overlap=1 << 31), dict(allow_self=2), dict(sires=[[1, 2]])):
        args = dict(offspring=[0], sires=[1, 2], dams=[2, 3])
        args.update(kw)
        with pytest.raises(ValueError):
            rcpp_api.parentage(M, (4, 6), **args)
        with pytest.raises(ValueError):
            rcpp_api.bed_parentage(bed, (4, 6), **args)
    tr = rcpp_api.mendel_trios("t", [[2, 0, 1], [2, 0, 1], [3, -1, 1], [3, -1, -1]], 4)
    assert tr.dtype == np.int32 and tr.flags["C_CONTIGUOUS"] and tr.shape == (4, 3)
    o, s, d, mo, selfing = rcpp_api.parentage_lists("t", [3, 0], [0, 1, 3], None, 4, 0, True)
    assert o.tolist() == [3, 0] and s.tolist() == [0, 1, 3] and d.size == 0 and d.dtype == np.int32 and (mo, selfing) == (0, 1)


def test_mendel_host_pieces_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mendel_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_mendel_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mendel host checks passed" in r.stdout


def test_the_two_chunk_loops_of_65535_are_where_the_gpu_cases_expect_them():
    """tests/test_gpu_regimes.py runs the second batch of both loops; a change here must move its cases."""
    flat = " ".join(re.sub(r"//.*", "", open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_mendel.hip")).read()).split())
    assert "for (long w0 = 0; w0 < nwords; w0 += 65535) {" in flat and "const long nw = nwords - w0 < 65535 ? nwords - w0 : 65535;" in flat
    assert "planes + w0 * np, np, nwords, nplanes, idx, cnt, cp, dst + w0 * cp);" in flat and "dim3((unsigned)(cp / 64), (unsigned)nw)" in flat
    assert "no > 65535" in flat and "const long oc = o0 + blockIdx.y;" in flat and "best_out + 8 * (o0 + (long)blockIdx.x) + 4 * lane" in flat
    ingest = " ".join(re.sub(r"//.*", "", open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ingest.cpp")).read()).split())
    assert "std::min(std::min(n_o, 65535L), ((long)1 << 28) / per)" in ingest and "for (long o0 = 0; o0 < n_o; o0 += chunk)" in ingest
    # the parentage search is the one caller of the gather, over all the panel's words at once; the trio pass never gathers
    assert ingest.count("eagle_dev_plane_gather(") == 1
    assert "eagle_dev_plane_gather(ctx, g.p(), g.nplanes, g.n, g.lp, sd.idx.as<int32_t>(), cnt, sd.sub.as<uint64_t>(), ctx->stream)" in ingest
