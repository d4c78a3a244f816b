"""CPU: the C ABI of the line scores without a device -- eagle_sample_scores and eagle_marker_scores are declared, exported and bound,
section 1b''''i of the header states the definitions, and every argument error is decided before a context is needed (ctx == NULL:
the text comes through eagle_open_error).  The rules behind those errors (csrc/eagle_host.h: scores_arg_error, score_digits) also run
in a stand-alone program under ASan + UBSan.  No device work."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
NAMES = ("eagle_sample_scores", "eagle_marker_scores")
MAX_LINE = 8388480


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_scores_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int and len(_lib.SIGNATURES[name][1]) == 7
    for macro, value in (("EAGLE_SCORES_MAX_COLUMNS", 64), ("EAGLE_SCORES_MAX_WEIGHT", 1 << 30), ("EAGLE_SCORES_MAX_LINE", MAX_LINE)):
        assert re.search(r"#define\s+%s\s+%dL?\b" % (macro, value), txt), macro
    assert MAX_LINE % 128 == 0 and MAX_LINE < 1 << 23 <= MAX_LINE + 128 and 128 * MAX_LINE < 1 << 31
    internal = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_internal.h")).read()
    assert re.search(r"\bint\s+eagle_dev_line_scores\s*\(\s*eagle_ctx\s*\*", internal) and hasattr(L, "eagle_dev_line_scores")
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_score.hip" in makefile and "eagle_score.o" in makefile
    assert (rcpp_api.SCORES_MAX_COLUMNS, rcpp_api.SCORES_MAX_WEIGHT, rcpp_api.SCORES_MAX_LINE) == (64, 1 << 30, MAX_LINE)


def test_header_states_the_definitions():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b''''i."):txt.index("1c. Dense")]
    for phrase in ("out[r T + t] = sum_c w[t C + c] g[r][c]", "|out| <= 2^30 C < 2^61", "g in {-1, 0, +1} = AA, AB, BB",
                   "a missing genotype of the source is a heterozygote", "|w| <= 2^30 = EAGLE_SCORES_MAX_WEIGHT", "1 <= T <= 64",
                   "w = d0 + 256 d1 + 256^2 d2 + 256^3 d3", "d in [-128, 127]", "d_p = ((w_p + 128) & 255) - 128", "w_{p+1} = (w_p - d_p) >> 8",
                   "Four digits hold every |w| <= 2^30", "costs nothing", "|w| <= 127 are one plane", "C <= EAGLE_SCORES_MAX_LINE = 8,388,480",
                   "largest multiple of 128 below 2^23", "128 C < 2^31", "no fold is needed", "do not depend on the order of summation",
                   "rectangular work list", "one pass over the image per call", "no temporary of image size", "are only read",
                   "bands of whole lines", "streamed and resident runs give the same integers", "VIEW alias", "dims[0] = kept entries",
                   "works on its first device", "decided before the context is used"):
        assert phrase in sec, phrase
    assert txt.index("1b''''.") < txt.index("1b''''i.") < txt.index("1c. Dense")


def test_scores_interface_is_public():
    import eagleeverything_amd
    from eagleeverything_amd import am, r_api, rcpp_api
    for name in ("line_scores_host", "score_digits_host", "quantise_weights", "Score", "ProjectPCA", "MarkerEffects", "Predict", "PCA"):
        assert callable(getattr(r_api, name))
    for name in ("blup_operands", "MarkerEffects", "Predict"):
        assert callable(getattr(am, name))
    p = inspect.signature(r_api.Score).parameters
    assert list(p)[:2] == ["geno", "weights"] and (p["include"].default, p["dosage"].default, p["availmemGb"].default, p["device"].default) == \
        (None, False, 8, 0)
    assert inspect.signature(r_api.PCA).parameters["loadings"].default is False
    assert inspect.signature(r_api.quantise_weights).parameters["bits"].default == 30
    assert list(inspect.signature(r_api.ProjectPCA).parameters)[:2] == ["pca", "geno"]
    assert list(inspect.signature(am.blup_operands).parameters) == ["y", "X", "K", "ve", "vg"]
    assert list(inspect.signature(am.MarkerEffects).parameters)[:4] == ["AMobj", "trait", "X", "geno"]
    p = inspect.signature(am.Predict).parameters
    assert list(p)[:3] == ["effects", "geno", "X"] and p["X"].default is None
    for fn in (rcpp_api.sample_scores, rcpp_api.marker_scores):
        p = inspect.signature(fn).parameters
        assert (p["max_memory_in_Gbytes"].default, p["device"].default) == (8.0, 0)
    for name in ("Score", "ProjectPCA", "MarkerEffects", "Predict"):
        assert name in eagleeverything_amd.__doc__


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()

    n, nm, T = 5, 7, 2
    out = (C.c_int64 * (max(n, nm) * 64))()
    names = ("path", "dims", "w", "T", "mem", "out")
    for fn, who, length in ((L.eagle_sample_scores, "sample_scores", nm), (L.eagle_marker_scores, "marker_scores", n)):
        by_marker = who == "marker_scores"
        w = (C.c_int32 * (64 * length))(*([3, -4] * (32 * length)))
        good = (str(tmp_path / "M.ascii").encode(), (C.c_long * 2)(n, nm), w, T, 8.0, out)

        def call(**kw):
            return fn(None, *[kw.get(k, v) for k, v in zip(names, good)])

        def dims(lines, line):           # (n, L) of M for a file of `lines` lines of `line` characters
            return (C.c_long * 2)(line, lines) if by_marker else (C.c_long * 2)(lines, line)
        assert call(path=None) == ERR_ARG and who in text() and "NULL" in text()
        assert call(dims=None) == ERR_ARG and "NULL" in text()
        assert call(w=None) == ERR_ARG and "NULL" in text()
        assert call(out=None) == ERR_ARG and "NULL" in text()
        assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
        assert call(dims=(C.c_long * 2)(n, -1)) == ERR_ARG and "dims" in text()
        assert call(T=0) == ERR_ARG and "T outside [1, 64]" in text()
        assert call(T=65) == ERR_ARG and "T outside [1, 64]" in text()
        assert call(T=-3) == ERR_ARG
        assert call(dims=dims(3, MAX_LINE + 1), T=1) == ERR_ARG and "EAGLE_SCORES_MAX_LINE" in text()      # a line of 8,388,481
        assert call(dims=dims(1 << 31, 1), T=1) == ERR_ARG and "2^31" in text()
        bad = (C.c_int32 * (T * length))(*([0] * (T * length)))
        bad[T * length - 1] = (1 << 30) + 1
        assert call(w=bad) == ERR_ARG and "2^30" in text()
        bad[T * length - 1] = -(1 << 30) - 1
        assert call(w=bad) == ERR_ARG and "2^30" in text()
        assert call() == ERR_ARG and "no context" in text()
        assert call(T=64) == ERR_ARG and "no context" in text()                                            # the limits themselves pass
        assert call(T=1) == ERR_ARG and "no context" in text()
        bad[T * length - 1] = 1 << 30
        bad[0] = -(1 << 30)
        assert call(w=bad) == ERR_ARG and "no context" in text()
        assert call(dims=dims((1 << 31) - 1, 1), T=1) == ERR_ARG and "no context" in text()
        long_w = np.zeros(MAX_LINE, dtype=np.int32)
        long_w[-1] = 1 << 30
        assert call(dims=dims(3, MAX_LINE), T=1, w=long_w.ctypes.data_as(C.POINTER(C.c_int32))) == ERR_ARG and "no context" in text()


def test_python_wrappers_refuse_before_the_library(tmp_path):
    from eagleeverything_amd import rcpp_api
    M, Mt = str(tmp_path / "M.ascii"), str(tmp_path / "Mt.ascii")          # no such files: a call that reached the library would say so
    n, nm = 4, 6
    for fn, path, length in ((rcpp_api.sample_scores, M, nm), (rcpp_api.marker_scores, Mt, n)):
        for w in (np.ones(length + 1, dtype=np.int64), np.ones((2, length - 1), dtype=np.int64), np.ones((2, 2, length), dtype=np.int64),
                  np.zeros((0, length), dtype=np.int64), np.full(length, 0.5), np.array([np.nan] + [1.0] * (length - 1)),
                  np.array([(1 << 30) + 1] + [0] * (length - 1)), np.array([-(1 << 30) - 1] + [0] * (length - 1)),
                  np.array(["a"] * length), np.full((65, length), 1 << 31)):
            with pytest.raises(ValueError):
                fn(path, (n, nm), w)


def test_scores_host_rules_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "scores_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_scores_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scores host checks passed" in r.stdout
