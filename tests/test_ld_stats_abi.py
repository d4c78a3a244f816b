"""CPU: the C ABI of LD scores and the LD decay curve without a device -- eagle_ld_stats and eagle_bed_ld_stats are declared, exported
and bound, section 1b'''v of the header states the definitions, and every argument error is decided before a context is needed
(ctx == NULL: the text comes through eagle_open_error).  The rule behind those errors (csrc/eagle_host.h: ld_stats_arg_error) also
runs in a stand-alone program under ASan + UBSan, built as tests/test_host_sanitizers.py builds its source.  No device work."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
NAMES = ("eagle_ld_stats", "eagle_bed_ld_stats")


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_ld_stats_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    assert len(_lib.SIGNATURES["eagle_ld_stats"][1]) == 14 and len(_lib.SIGNATURES["eagle_bed_ld_stats"][1]) == 16
    internal = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_internal.h")).read()
    assert re.search(r"\bint\s+eagle_dev_ld_reduce\s*\(\s*eagle_ctx\s*\*", internal) and hasattr(L, "eagle_dev_ld_reduce")
    for py in ("ld_stats", "bed_ld_stats"):
        assert callable(getattr(rcpp_api, py))
    assert rcpp_api.LD_STATS_MAX_BINS == 512


def test_header_states_the_definitions():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b'''v."):txt.index("1b''''.")]
    for phrase in ("u_ij = (uint64)(r2_ij 1073741824.0)", "the conversion truncates", "c^2 <= v_i v_j in integers", "rounding is monotone",
                   "equal products round equally", "do not depend on the order of summation", "1 <= |j - i| <= window <= 256",
                   "chrom[i] == chrom[j]", "|pos[j] - pos[i]| <= max_dist", "need not be sorted", "1.0 + (double)U_i 2^-30",
                   "U = 0, cnt = 0 and score 1.0", "edges[b] <= d_ij < edges[b + 1]", "1 <= B <= 512", "still counts in the scores",
                   "(double)sum / (double)pairs 2^-30", "markers window <= 2^33", "no bin sum can pass 2^63",
                   "does not depend on the window size", "decided before the context is used"):
        assert phrase in sec, phrase
    assert txt.index("1b'''iv.") < txt.index("1b'''v.") < txt.index("1b''''.")


def test_ld_stats_interface_is_public():
    from eagleeverything_amd import r_api, rcpp_api
    for name in ("ld_band_host", "ld_stats_host", "ld_half_decay", "LDScore", "LDDecay"):
        assert callable(getattr(r_api, name))
    p = inspect.signature(r_api.LDScore).parameters
    assert (p["window"].default, p["map"].default, p["kb"].default, p["bed"].default, p["include"].default, p["min_overlap"].default) == \
        (50, None, None, None, None, 1)
    p = inspect.signature(r_api.LDDecay).parameters
    assert (p["window"].default, p["map"].default, p["bins"].default, p["kb"].default, p["bed"].default) == (256, None, None, None, None)
    assert list(inspect.signature(r_api.ld_stats_host).parameters) == ["band", "chrom", "pos", "max_dist", "edges"]
    assert list(inspect.signature(r_api.ld_band_host).parameters) == ["Mt8", "window"]
    for fn in (r_api.grm_weights, r_api.GRM, r_api.PCA):
        assert inspect.signature(fn).parameters["ld_score"].default is None
    p = inspect.signature(rcpp_api.ld_stats).parameters
    assert (p["window"].default, p["chrom"].default, p["pos"].default, p["max_dist"].default, p["edges"].default) == (50, None, None, 0, None)
    p = inspect.signature(rcpp_api.bed_ld_stats).parameters
    assert (p["window"].default, p["include"].default, p["min_overlap"].default, p["edges"].default) == (50, None, 1, None)


def i64(*v):
    return (C.c_int64 * len(v))(*v)


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()

    nm = 7
    dims = (C.c_long * 2)(5, nm)
    U, cnt = (C.c_uint64 * nm)(), (C.c_int32 * nm)()
    bsum, bpairs = (C.c_uint64 * 512)(), (C.c_int64 * 512)()
    chrom, pos = (C.c_int32 * nm)(), (C.c_int64 * nm)()
    edges = i64(1, 3, 6)
    full = i64(*range(513))

    fn = L.eagle_ld_stats
    good = (str(tmp_path / "Mt.ascii").encode(), dims, 50, chrom, pos, 2000, edges, 2, 8.0, U, cnt, bsum, bpairs)
    names = ("path", "dims", "window", "chrom", "pos", "max_dist", "edges", "nbins", "mem", "U", "cnt", "bsum", "bpairs")

    def call(**kw):
        return fn(None, *[kw.get(k, v) for k, v in zip(names, good)])
    assert call(path=None) == ERR_ARG and "ld_stats" in text() and "NULL" in text()
    assert call(dims=None) == ERR_ARG
    assert call(U=None) == ERR_ARG
    assert call(cnt=None) == ERR_ARG
    assert call(bsum=None) == ERR_ARG and "NULL" in text()                               # edges given: the bin outputs are needed
    assert call(bpairs=None) == ERR_ARG
    assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(5, -1)) == ERR_ARG
    assert call(window=0) == ERR_ARG and "window" in text()
    assert call(window=257) == ERR_ARG
    assert call(dims=(C.c_long * 2)(5, 1 << 31)) == ERR_ARG and "2^31" in text()
    assert call(dims=(C.c_long * 2)(5, (1 << 25) + 1), window=256) == ERR_ARG and "2^33" in text()     # definition 6
    assert call(dims=(C.c_long * 2)(5, (1 << 31) - 1), window=5) == ERR_ARG and "2^33" in text()
    assert call(pos=None) == ERR_ARG and "max_dist needs pos" in text()
    assert call(nbins=-1) == ERR_ARG and "nbins" in text()
    assert call(nbins=513) == ERR_ARG
    assert call(edges=i64(1, 3, 3)) == ERR_ARG and "strictly increasing" in text()
    assert call(edges=i64(4, 3, 6)) == ERR_ARG
    assert call() == ERR_ARG and "no context" in text()
    assert call(dims=(C.c_long * 2)(5, 1 << 25), window=256, edges=full, nbins=512) == ERR_ARG and "no context" in text()      # the limits themselves pass
    assert call(dims=(C.c_long * 2)(5, (1 << 31) - 1), window=4) == ERR_ARG and "no context" in text()
    assert call(chrom=None, pos=None, max_dist=0) == ERR_ARG and "no context" in text()
    assert call(pos=None, max_dist=-1) == ERR_ARG and "no context" in text()             # max_dist <= 0: no distance limit
    assert call(edges=None, bsum=None, bpairs=None) == ERR_ARG and "no context" in text()          # no decay: the bin outputs may be NULL
    assert call(nbins=0, bsum=None, bpairs=None) == ERR_ARG and "no context" in text()

    fn = L.eagle_bed_ld_stats
    include = (C.c_uint8 * nm)(1, 0, 1, 1, 0, 1, 1)
    good = (str(tmp_path / "p.bed").encode(), dims, include, 50, 1, chrom, pos, 2000, edges, 2, 8.0, U, cnt, bsum, bpairs)
    names = ("path", "dims", "include", "window", "min_overlap", "chrom", "pos", "max_dist", "edges", "nbins", "mem", "U", "cnt", "bsum", "bpairs")
    assert call(path=None) == ERR_ARG and "bed_ld_stats" in text() and "NULL" in text()
    assert call(dims=None) == ERR_ARG
    assert call(U=None) == ERR_ARG
    assert call(cnt=None) == ERR_ARG
    assert call(bsum=None) == ERR_ARG
    assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
    assert call(dims=(C.c_long * 2)(1 << 30, nm)) == ERR_ARG and "2^30" in text()
    assert call(min_overlap=0) == ERR_ARG and "min_overlap" in text()
    assert call(include=(C.c_uint8 * nm)()) == ERR_ARG and "no marker" in text()
    assert call(window=0) == ERR_ARG and "window" in text()
    assert call(window=257) == ERR_ARG
    assert call(include=None, dims=(C.c_long * 2)(5, 1 << 31)) == ERR_ARG and "2^31" in text()
    assert call(include=None, dims=(C.c_long * 2)(5, (1 << 25) + 1), window=256) == ERR_ARG and "2^33" in text()
    assert call(pos=None) == ERR_ARG and "max_dist needs pos" in text()
    assert call(nbins=513) == ERR_ARG and "nbins" in text()
    assert call(nbins=-2) == ERR_ARG
    assert call(edges=i64(1, 1, 6)) == ERR_ARG and "strictly increasing" in text()
    assert call() == ERR_ARG and "no context" in text()
    assert call(include=None, window=256, edges=full, nbins=512, min_overlap=5) == ERR_ARG and "no context" in text()
    assert call(chrom=None, pos=None, max_dist=0, edges=None, bsum=None, bpairs=None) == ERR_ARG and "no context" in text()


def test_python_wrappers_refuse_before_the_library(tmp_path):
    from eagleeverything_amd import rcpp_api
    Mt, bed = str(tmp_path / "Mt.ascii"), str(tmp_path / "a.bed")
    for kw in (dict(chrom=[1, 1, 2]), dict(chrom=[1, 1.5, 2, 2, 2, 2]), dict(pos=[1, 2, 3]), dict(pos=[1, 2, 3, 4, 5, 6.5]), dict(max_dist=10),
               dict(edges=[1]), dict(edges=[1, 1]), dict(edges=[1, 2.5]), dict(edges=list(range(514)))):
        with pytest.raises(ValueError):
            rcpp_api.ld_stats(Mt, (4, 6), **kw)
        with pytest.raises(ValueError):
            rcpp_api.bed_ld_stats(bed, (4, 6), **kw)
    with pytest.raises(ValueError):
        rcpp_api.bed_ld_stats(bed, (4, 6), include=[1, 0, 1])
    with pytest.raises(ValueError):
        rcpp_api.bed_ld_stats(bed, (4, 6), include=[1, 0, 1, 0, 1, 0], chrom=np.zeros(6))                  # chrom is by PANEL marker


def test_ld_stats_argument_rule_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ld_stats_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_ld_stats_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ld stats host checks passed" in r.stdout
