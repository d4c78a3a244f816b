"""CPU: marker QC without a device -- the three entry points are declared, exported and bound; the host rules (statistics from
integer counts, PLINK's keep rules) on hand-made count tables; the committed fixture's truth; argument errors that are decided
before a device is needed.  Expected values are numpy restatements written here; every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

NAMES = ("eagle_marker_counts", "eagle_bed_marker_counts", "eagle_filter_markers")
ERR_ARG = -3


# ------------------------------------------------------------------------------------------------ 1. the ABI
def test_qc_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eagle_hip.h")).read(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    assert len(_lib.SIGNATURES["eagle_filter_markers"][1]) == 10
    for py in ("marker_counts", "bed_marker_counts", "filter_markers"):
        assert callable(getattr(rcpp_api, py))


def test_qc_interface_is_public():
    from eagleeverything_amd import r_api
    for name in ("MarkerStats", "FilterMarkers", "subset_map", "marker_stats_from_counts", "marker_keep_mask"):
        assert callable(getattr(r_api, name))
    import inspect
    p = inspect.signature(r_api.ReadMarker).parameters
    assert p["maf"].default is None and p["max_missing"].default is None and p["drop_monomorphic"].default is False


# ------------------------------------------------------------------------------------------------ 2. the host rules
def test_stats_from_counts_by_hand():
    from eagleeverything_amd import r_api
    #                 plain       with missing   all missing   monomorphic 0   monomorphic 2   all het
    n0 = np.array([50, 10, 0, 100, 0, 0])
    n1 = np.array([40, 20, 0, 0, 0, 100])
    n2 = np.array([10, 50, 0, 0, 100, 0])
    nm = np.array([0, 20, 100, 0, 0, 0])
    st = r_api.marker_stats_from_counts(n0, n1, n2, nm)
    assert all(st[k].shape == (6,) for k in ("n0", "n1", "n2", "n_missing", "freq", "maf", "het", "call_rate"))
    assert np.array_equal(st["n_missing"], nm) and np.array_equal(st["n1"], n1)
    # freq = (2 n2 + n1) / (2 n_called): the missing genotypes are in neither count
    assert st["freq"][0] == 60 / 200 and st["freq"][1] == 120 / 160 and st["freq"][3] == 0.0 and st["freq"][4] == 1.0 and st["freq"][5] == 0.5
    assert st["maf"][0] == 60 / 200 and st["maf"][1] == 40 / 160 and st["maf"][3] == 0.0 and st["maf"][4] == 0.0 and st["maf"][5] == 0.5
    assert st["het"][0] == 40 / 100 and st["het"][1] == 20 / 80 and st["het"][5] == 1.0
    assert st["call_rate"][0] == 1.0 and st["call_rate"][1] == 80 / 100 and st["call_rate"][2] == 0.0
    assert np.isnan(st["freq"][2]) and np.isnan(st["maf"][2]) and np.isnan(st["het"][2])
    # without a missing column: zeros
    st0 = r_api.marker_stats_from_counts(n0, n1, n2)
    assert not st0["n_missing"].any() and st0["call_rate"][0] == 1.0


def test_keep_mask_boundaries_and_rules():
    from eagleeverything_amd import r_api
    # n = 100 individuals.  maf: 10/200 = 0.05 exactly (kept at 0.05), 9/200 (dropped), the same two from the other allele's side
    n2 = np.array([0, 0, 95, 96, 0, 50, 0])
    n1 = np.array([10, 9, 0, 0, 0, 0, 0])
    n0 = np.array([90, 91, 5, 4, 100, 30, 0])
    nm = np.array([0, 0, 0, 0, 0, 20, 100])      # marker 5: 20 % missing; marker 6: no call at all
    st = r_api.marker_stats_from_counts(n0, n1, n2, nm)
    assert st["maf"][0] == 0.05 and st["maf"][2] == 0.05
    keep = r_api.marker_keep_mask
    assert keep(st).all()                                                              # no filter switched on: everything stays
    assert keep(st, maf=0.05).tolist() == [True, False, True, False, False, True, False]
    assert keep(st, max_missing=0.2).tolist() == [True] * 6 + [False]                  # 20/100 == 0.2 exactly: kept
    assert keep(st, max_missing=0.19).tolist() == [True] * 5 + [False, False]
    assert keep(st, drop_monomorphic=True).tolist() == [True, True, True, True, False, True, False]
    assert keep(st, maf=0.05, max_missing=0.1, drop_monomorphic=True).tolist() == [True, False, True, False, False, False, False]
    assert keep(st, maf=0.0).tolist() == [True] * 6 + [False]                          # the all-missing marker goes with ANY filter


def test_subset_map_on_bim_dict_and_list(tmp_path):
    from eagleeverything_amd import r_api
    bim = r_api.ReadBim(os.path.join(GOLDEN, "plink_150x100.bim"))
    geno = {"asciifileM": "M", "asciifileMt": "Mt", "dim_of_ascii_M": [150, 3], "marker_index": np.array([2, 40, 99])}
    sub = r_api.subset_map(bim, geno)
    assert sub == {"SNP": [bim["SNP"][i] for i in (2, 40, 99)], "Chr": [bim["Chr"][i] for i in (2, 40, 99)],
                   "Pos": [bim["Pos"][i] for i in (2, 40, 99)]}
    names = ["m%d" % j for j in range(100)]
    assert r_api.subset_map(names, geno) == ["m2", "m40", "m99"]
    plain = {"asciifileM": "M", "asciifileMt": "Mt", "dim_of_ascii_M": [150, 100]}
    assert r_api.subset_map(names, plain) is names and r_api.subset_map(None, geno) is None


# ------------------------------------------------------------------------------------------------ 3. the committed fixture
def _fixture_truth():
    D = np.loadtxt(os.path.join(GOLDEN, "geno_150x100.txt"), dtype=np.int64)     # digits, n x L
    assert D.shape == (150, 100) and set(np.unique(D)) == {0, 1, 2}
    c = np.stack([np.sum(D == v, axis=0) for v in (0, 1, 2)], axis=1)
    a2 = 2 * c[:, 2] + c[:, 1]
    return D, c, np.minimum(a2, 300 - a2) / 300.0


def test_fixture_truth_and_host_rule():
    from eagleeverything_amd import r_api
    D, c, maf = _fixture_truth()
    assert maf.min() > 0 and round(maf.min(), 4) == 0.0133 and round(maf.max(), 3) == 0.497     # no monomorphic marker
    st = r_api.marker_stats_from_counts(c[:, 0], c[:, 1], c[:, 2])
    assert np.array_equal(st["maf"], maf) and np.array_equal(st["het"], c[:, 1] / 150.0) and np.all(st["call_rate"] == 1.0)
    for thr, dropped in ((0.05, 7), (0.1, 24)):
        truth = maf >= thr
        assert int((~truth).sum()) == dropped
        assert np.array_equal(r_api.marker_keep_mask(st, maf=thr), truth)
    assert r_api.marker_keep_mask(st, drop_monomorphic=True).all()


# ------------------------------------------------------------------------------------------------ 4. errors that need no device
def _call_filter(L, keep, fM, fMt, oM, oMt, dims=(150, 100)):
    from eagleeverything_amd._lib import c_lp
    kv = np.asarray(keep, dtype=np.int64)
    out = (C.c_long * 2)()
    rc = L.eagle_filter_markers(None, os.fsencode(fM), os.fsencode(fMt), (C.c_long * 2)(*dims), kv.ctypes.data_as(c_lp), kv.size,
                                os.fsencode(oM), os.fsencode(oMt), 8.0, out)
    return rc, L.eagle_open_error().decode()


def test_filter_markers_argument_errors_without_a_device(tmp_path):
    from eagleeverything_amd import _lib, rcpp_api
    L = _lib.load()
    fM, fMt = str(tmp_path / "M.ascii"), str(tmp_path / "Mt.ascii")
    oM, oMt = str(tmp_path / "oM.ascii"), str(tmp_path / "oMt.ascii")
    for keep, word in (([3, 2, 5], "strictly increasing"), ([1, 1], "strictly increasing"), ([0, 100], "outside"), ([-1, 4], "outside"),
                       ([], "empty")):
        rc, text = _call_filter(L, keep, fM, fMt, oM, oMt)
        assert rc == ERR_ARG and word in text, (keep, text)
    for a, b in ((fM, oMt), (oM, fMt), (fMt, oMt), (oM, fM), (oM, oM)):
        rc, text = _call_filter(L, [0, 1], fM, fMt, a, b)
        assert rc == ERR_ARG and "must differ" in text
    rc, text = _call_filter(L, [0, 1], fM, fMt, oM, oMt)          # a good argument list gets as far as asking for the context
    assert rc == ERR_ARG and "no context" in text
    if 0 not in rcpp_api._ctx:   # the Python binding reports the same errors without opening a device
        with pytest.raises(rcpp_api.EagleError) as e:
            rcpp_api.filter_markers(fM, fMt, (150, 100), [5, 4], oM, oMt)
        assert e.value.code == ERR_ARG and "strictly increasing" in e.value.text
        with pytest.raises(rcpp_api.EagleError) as e:
            rcpp_api.filter_markers(fM, fMt, (150, 100), [4, 5], fM, oMt)
        assert e.value.code == ERR_ARG
    assert sorted(os.listdir(tmp_path)) == []                      # nothing was written
    for fn, args in ((L.eagle_marker_counts, (b"Mt.ascii",)), (L.eagle_bed_marker_counts, (b"x.bed",))):
        buf = (C.c_int32 * 12)()
        assert fn(None, *args, (C.c_long * 2)(0, 4), 8.0, buf) == ERR_ARG and "positive" in L.eagle_open_error().decode()
        assert fn(None, *args, (C.c_long * 2)(3, 4), 8.0, buf) == ERR_ARG and "no context" in L.eagle_open_error().decode()


def test_filter_markers_host_exits_with_given_stats(tmp_path):
    """With stats= handed in, FilterMarkers decides these three cases on the host: nothing dropped, nothing kept, a bad outdir."""
    from eagleeverything_amd import r_api
    D, c, maf = _fixture_truth()
    st = r_api.marker_stats_from_counts(c[:, 0], c[:, 1], c[:, 2])
    src = tmp_path / "src"
    src.mkdir()
    geno = {"asciifileM": str(src / "M.ascii"), "asciifileMt": str(src / "Mt.ascii"), "dim_of_ascii_M": [150, 100]}
    same = r_api.FilterMarkers(geno, maf=0.01, stats=st)
    assert {k: same[k] for k in geno} == geno and np.array_equal(same["marker_index"], np.arange(100)) and same["marker_index"].dtype == np.int64
    same = r_api.FilterMarkers(geno, drop_monomorphic=True, stats=st)
    assert np.array_equal(same["marker_index"], np.arange(100))
    msgs = []
    assert r_api.FilterMarkers(geno, maf=0.6, stats=st, message=msgs.append) is None and any("no marker passes" in m for m in msgs)
    msgs = []
    assert r_api.FilterMarkers(geno, maf=0.05, stats=st, outdir=str(src), message=msgs.append) is None
    assert any("directory of their own" in m for m in msgs)
    assert os.listdir(src) == [] and not (src / "qc").exists()
