"""CPU: the C ABI of the per-group counts and Fisher's exact test without a device -- eagle_group_counts, eagle_bed_group_counts and
eagle_fisher_2x2 are declared, exported and bound, section 1b''''iii of the header states the definition, the invariants and the order
of the Fisher walk, every argument error is decided before a context is needed (ctx == NULL: the text comes through
eagle_open_error), and the Python wrappers refuse malformed input before the library is called.  No device work."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
NAMES = {"eagle_group_counts": 7, "eagle_bed_group_counts": 7, "eagle_fisher_2x2": 4}


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_group_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name, nargs in NAMES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int and len(_lib.SIGNATURES[name][1]) == nargs
    assert re.search(r"#define EAGLE_GROUPS_MAX 64\b", txt) and rcpp_api.GROUPS_MAX == 64
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_groups.hip" in makefile and "eagle_groups.o" in makefile
    kern = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_groups.hip")).read()
    code = re.sub(r"//.*", "", kern)
    for k in ("k_group_onehot", "k_group_tile", "k_bed_group_counts", "k_fisher_2x2"):
        assert k in code, k
    assert "__builtin_amdgcn_mfma_i32_32x32x32_i8" in code and "0x01010101" in code and "asm" not in code and "atomic" not in code
    for piece in ("__dmul_rn", "__ddiv_rn", "__dadd_rn", "1.0000001"):
        assert piece in code, piece
    ctxh = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ctx.h")).read()
    for name in ("eagle_dev_group_onehot", "eagle_dev_group_counts", "eagle_dev_bed_group_counts", "eagle_dev_fisher_2x2"):
        assert name in ctxh and hasattr(L, name), name


def test_header_states_the_definition():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b''''iii."):txt.index("1c.")]
    for phrase in ("labels[i] in {-1, 0, ..., K - 1}", "1 <= K <= EAGLE_GROUPS_MAX = 64", "one per kept individual",
                   "a missing call of the source is a heterozygote", "n2 = (q + s) / 2, n0 = (q - s) / 2, n1 = size_k - q",
                   "counts_out[(m K + k) 3 + c]", "counts_out[(m K + k) 4 + c]", "The unused bit pairs of a row's last byte are not counted",
                   "eagle_marker_counts / eagle_bed_marker_counts exactly", "K = 1 with all labels 0 IS those calls",
                   "x0 = clamp(floor((r1 + 1) (c1 + 1) / (N + 2)), lo, hi)", "P(x - 1) = P(x) x (r2 - c1 + x) / ((r1 - x + 1) (c1 - x + 1))",
                   "P(x + 1) = P(x) (r1 - x) (c1 - x) / ((x + 1) (r2 - c1 + x + 1))", "exact int64 products converted to fp64 once",
                   "cut = fl(P(a) 1.0000001)", "p = min(1, fl(tail / total))", "R's fisher.test", "N = 0 gives p = 1",
                   "Agreement with the PLINK program is neither claimed nor tested", "a multi-device context works on its first device",
                   "decided before the context is used", "a table sum above 2^30", "n > 2^30 - 1"):
        assert phrase in sec, phrase
    assert txt.index("1b''''ii.") < txt.index("1b''''iii.") < txt.index("1c.")
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "GroupCounts" in readme and "CaseControl" in readme and "agreement with the PLINK program is neither claimed nor tested" in readme


def test_group_interface_is_public():
    import eagleeverything_amd
    from eagleeverything_amd import r_api, rcpp_api
    assert eagleeverything_amd.__all__ == ["rcpp_api", "r_api", "host_model", "synth"]
    for name in ("group_labels", "group_counts_host", "bed_group_counts_host", "fisher_2x2_host", "GroupCounts", "Fst", "CaseControl",
                 "fst_from_counts", "case_control_from_counts"):
        assert callable(getattr(r_api, name)), name
    assert list(inspect.signature(rcpp_api.group_counts).parameters)[:4] == ["f_name_ascii_Mt", "dims", "labels", "K"]
    assert list(inspect.signature(rcpp_api.bed_group_counts).parameters)[:4] == ["bed_path", "dims", "labels", "K"]
    assert list(inspect.signature(rcpp_api.fisher_2x2).parameters)[:1] == ["tables"]
    p = inspect.signature(r_api.Fst).parameters
    assert [(k, p[k].default) for k in list(p)[2:7]] == [("method", "hudson"), ("bed", None), ("map", None), ("window", None), ("kb", None)]
    p = inspect.signature(r_api.CaseControl).parameters
    assert [(k, p[k].default) for k in list(p)[2:4]] == [("bed", None), ("fisher", False)]
    p = inspect.signature(r_api.GroupCounts).parameters
    assert [(k, p[k].default) for k in list(p)[2:4]] == [("bed", None), ("include", None)]
    assert "HWE(out[\"counts\"][:, k])" in r_api.GroupCounts.__doc__ and "controls" in r_api.GroupCounts.__doc__


def test_python_wrappers_refuse_before_the_library(tmp_path, monkeypatch):
    from eagleeverything_amd import _lib, r_api, rcpp_api
    Mt = str(tmp_path / "Mt.ascii")
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    for fn in (rcpp_api.group_counts, rcpp_api.bed_group_counts):
        for labels, K in (([0, 1, 0], None), ([0, 1, 0, 1, 0, 1, 0], None), ([0, 0.5, 1, 0, 1, 0], None), ([0, 1, 2, 0, 1, 2], 2),
                          ([0, -2, 1, 0, 1, 0], None), ([0, 1, 0, 1, 0, float("nan")], None), ([[0, 1, 0], [1, 0, 1]], None),
                          ([0, 1, 0, 1, 0, 1], 0), (["a", "b", "a", "b", "a", "b"], None)):
            with pytest.raises(ValueError):
                fn(Mt, (6, 4), labels, K)
    for t in ([1, 2, 3, 4], [[1, 2, 3]], [[1, 2, 3, 4.5]], [[1, -2, 3, 4]], [[1 << 29, 1 << 29, 1, 0]], np.zeros((0, 4))):
        with pytest.raises(ValueError):
            rcpp_api.fisher_2x2(t)
    geno = {"asciifileM": str(tmp_path / "M.ascii"), "asciifileMt": Mt, "dim_of_ascii_M": [6, 4]}
    with pytest.raises(ValueError):
        r_api.GroupCounts(geno, ["a", "b", "a"])
    with pytest.raises(ValueError):
        r_api.CaseControl(geno, [0, 1, 2, 0, 1, 0])
    with pytest.raises(ValueError):
        r_api.CaseControl(geno, [0, 1, 0])
    with pytest.raises(ValueError):
        r_api.Fst(geno, ["a", "b", "a", "b", "a", "b"], kb=5)


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib, rcpp_api
    L = _lib.load()
    i32p = C.POINTER(C.c_int32)

    def text():
        return L.eagle_open_error().decode()

    n, nm = 6, 9
    dims, path = (C.c_long * 2)(n, nm), os.fsencode(str(tmp_path / "nothing"))
    lab = (C.c_int32 * n)(0, 1, -1, 0, 1, 1)
    out = (C.c_int32 * (nm * 2 * 4))()
    for fn, who in ((L.eagle_group_counts, "group_counts"), (L.eagle_bed_group_counts, "bed_group_counts")):
        for args in ((None, dims, lab, 2, 8.0, out), (path, None, lab, 2, 8.0, out), (path, dims, None, 2, 8.0, out),
                     (path, dims, lab, 2, 8.0, None)):
            assert fn(None, *args) == ERR_ARG and text() == who + ": NULL argument"
        for bad in ((0, nm), (n, 0), (-1, nm)):
            assert fn(None, path, (C.c_long * 2)(*bad), lab, 2, 8.0, out) == ERR_ARG and text() == who + ": dims must be positive"
        # decided before a single label is read: the six labels above are all there is
        assert fn(None, path, (C.c_long * 2)(1 << 30, nm), lab, 2, 8.0, out) == ERR_ARG and "2^30 - 1" in text()
        for K in (0, -1, 65):
            assert fn(None, path, dims, lab, K, 8.0, out) == ERR_ARG and text() == who + ": K outside [1, 64]"
        assert fn(None, path, dims, lab, 1, 8.0, out) == ERR_ARG and text() == who + ": a label outside [-1, K)"        # label 1 with K = 1
        assert fn(None, path, dims, (C.c_int32 * n)(0, 1, -2, 0, 1, 1), 2, 8.0, out) == ERR_ARG and "a label outside" in text()
        assert fn(None, path, dims, lab, 2, 8.0, out) == ERR_ARG and text() == who + ": no context"                   # nothing wrong but the context
        assert fn(None, path, dims, lab, 64, 8.0, out) == ERR_ARG and text() == who + ": no context"
    p = (C.c_double * 2)()
    good = (C.c_int32 * 8)(1, 2, 3, 4, 0, 0, 0, 0)
    assert L.eagle_fisher_2x2(None, None, 2, p) == ERR_ARG and "NULL" in text()
    assert L.eagle_fisher_2x2(None, good, 2, None) == ERR_ARG and "NULL" in text()
    assert L.eagle_fisher_2x2(None, good, 0, p) == ERR_ARG and "positive" in text()
    assert L.eagle_fisher_2x2(None, (C.c_int32 * 8)(1, 2, 3, 4, 0, -1, 0, 0), 2, p) == ERR_ARG and "negative" in text()
    assert L.eagle_fisher_2x2(None, (C.c_int32 * 8)(1, 2, 3, 4, 1 << 29, 1 << 29, 1, 0), 2, p) == ERR_ARG and "2^30" in text()
    assert L.eagle_fisher_2x2(None, (C.c_int32 * 8)(1, 2, 3, 4, 1 << 29, 1 << 29, 0, 0), 2, p) == ERR_ARG and "no context" in text()
    # through the wrappers an argument error of the library arrives as EagleError(-3) and opens no device
    import torch
    if not torch.cuda.is_available():
        assert not rcpp_api._ctx
    with pytest.raises(rcpp_api.EagleError) as e:
        rcpp_api.group_counts(str(tmp_path / "nothing"), (0, 4), [])
    assert e.value.code == ERR_ARG and "dims must be positive" in e.value.text
    with pytest.raises(rcpp_api.EagleError) as e:
        rcpp_api.bed_group_counts(str(tmp_path / "nothing"), (3, 0), [0, 1, 0])
    assert e.value.code == ERR_ARG and "dims must be positive" in e.value.text
