"""GPU: the HIP entry points against what the REFERENCE's own src/*.cpp wrote (tests/golden/ref_<case>.npz, recorded by
tests/golden/make_ref_golden.py from oracle/_ref; kept honest by test_oracle_vs_reference.py on a machine that has the reference).
No oracle and no reference checkout take part here.

Integer and byte outputs: exact.  a, vara, tsq: the gates smoke() and the README state -- a within rtol 1e-9 (atol 1e-12 max|a|),
vara within 1e-7, tsq within 1e-6, the selected marker identical -- measured against the reference's long-double values.
"""
import json
import os

import numpy as np
import pytest

import refpin
from refpin import ALL_CASES, GOLDEN_CASES, NA
from eagleeverything_amd import host_model, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from eagleeverything_amd import rcpp_api
    assert rcpp_api.device_info()["arch"].startswith("gfx950")
    yield rcpp_api
    rcpp_api.close_all()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    out = {}
    for case in ALL_CASES:
        g = refpin.case_inputs(case)
        d = tmp_path_factory.mktemp(case)
        rec = dict(np.load(os.path.join(refpin.GOLDEN, "ref_%s.npz" % case), allow_pickle=False))
        rec["texts"], rec["digests"] = json.loads(str(rec["texts_json"])), json.loads(str(rec["digests_json"]))
        out[case] = (g, synth.write_geno_pair(str(d), np.ascontiguousarray(g["M8"].T)), rec, d)
    return out


def _which_max(a, vara):
    """which(tsq == max(tsq, na.rm=TRUE))[1] of find_qtl.R:71-83, 1-based."""
    with np.errstate(all="ignore"):
        tsq = np.ravel(a) ** 2 / np.ravel(vara)
    return int(np.flatnonzero(tsq == np.nanmax(tsq))[0]) + 1, tsq


def _check_scan(res, a_ld, vara_ld, idx=None, a_rtol=1e-9, vara_rtol=1e-7, tsq_rtol=1e-6, label=""):
    a, vara = np.ravel(res["a"]), np.ravel(res["vara"])
    assert a.shape == a_ld.shape and vara.shape == vara_ld.shape, label
    np.testing.assert_allclose(a, a_ld, rtol=a_rtol, atol=1e-12 * np.abs(a_ld).max(), err_msg=label)
    # markers constant over individuals have vara == 0 up to rounding noise: an absolute floor of 1e-12 max|vara|, as in
    # test_gpu_parity.test_scan_matches_oracle
    np.testing.assert_allclose(vara, vara_ld, rtol=vara_rtol, atol=1e-12 * np.abs(vara_ld).max(), err_msg=label)
    np.testing.assert_array_equal(vara == 0.0, vara_ld == 0.0, err_msg=label)            # the same rows masked
    idx_ref, tsq_ref = _which_max(a_ld, vara_ld)
    _, tsq = _which_max(a, vara)
    ok = np.isfinite(tsq_ref) & (tsq_ref > 0) & (np.abs(vara_ld) > 1e-8 * np.median(np.abs(vara_ld)))
    assert np.max(np.abs(tsq[ok] - tsq_ref[ok]) / tsq_ref[ok]) <= tsq_rtol, label
    assert _which_max(a, vara)[0] == idx_ref, label
    if idx is not None:
        assert idx == idx_ref, label


@pytest.mark.parametrize("case", ALL_CASES)
def test_exact_outputs(case, cases, api):
    g, geno, rec, _ = cases[case]
    n, L = g["M8"].shape
    fM, fMt = geno["asciifileM"], geno["asciifileMt"]
    np.testing.assert_array_equal(api.ReadBlock(fMt, 7, n - 5, 11), rec["readblock_Mt_7"].astype(np.float64))
    np.testing.assert_array_equal(api.ReadBlock(fM, n - 1, L, 1), rec["readblock_M_last"].astype(np.float64))
    sel = rec["sel_masked"]
    np.testing.assert_array_equal(sel, refpin.masked_pair(L))
    need = (n * n * 8 + 2 * n * L * 8) / 1e9
    for mem in (8.0, need / 6.0):
        np.testing.assert_array_equal(api.calculateMMt_rcpp(fM, mem, 2, NA, (n, L)), rec["MMt"].astype(np.float64))
        np.testing.assert_array_equal(api.calculateMMt_rcpp(fM, mem, 2, sel, (n, L)), rec["MMt_masked"].astype(np.float64))
    msgs = []
    api.calculateMMt_rcpp(fM, 8.0, 2, sel, (n, L), message=msgs.append)
    assert msgs == rec["texts"]["mmt_messages"]
    for quiet, tag in ((True, "quiet"), (False, "loud")):   # the row-block branch: its two lines come whatever `quiet` is
        msgs = []
        api.calculateMMt_rcpp(fM, need / 6.0, 2, NA, (n, L), quiet=quiet, message=msgs.append)
        assert len(rec["texts"]["mmt_block_messages_" + tag]) == 3 and msgs == rec["texts"]["mmt_block_messages_" + tag], tag
    for c, exp in zip(rec["extract_loci"], rec["extract"]):
        np.testing.assert_array_equal(api.extract_geno_rcpp(fM, 8.0, int(c), (n, L)), exp)
    api.drop_cache()


@pytest.mark.parametrize("wmode", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", ALL_CASES)
def test_scan_against_the_reference(case, mode, wmode, cases, api, request, monkeypatch):
    g, geno, rec, _ = cases[case]
    n, L = g["M8"].shape
    fM, fMt = geno["asciifileM"], geno["asciifileMt"]

    def restore():
        api.set_scan_mode(1)
        api.set_w_mode(1)
        api.drop_cache()
    request.addfinalizer(restore)
    api.set_scan_mode(mode)
    api.set_w_mode(wmode)
    for tag, sel in (("na", NA), ("masked", rec["sel_masked"])):
        a_ld, vara_ld = rec["a_%s_ld" % tag], rec["vara_%s_ld" % tag]
        res = api.calculate_a_and_vara_rcpp(fMt, sel, g["S"], g["V"], 8.0, (L, n), g["ahat"])
        assert res["a"].shape == (L, 1)
        _check_scan(res, a_ld, vara_ld, idx=api.last_scan_argmax()[0], label="resident " + tag)
        if tag == "masked":
            for s in rec["sel_masked"].astype(int):
                assert res["a"][s, 0] == 0.0 and res["vara"][s, 0] == 0.0
    # the sentinel exit of a negative budget: List(a=0, vara=0) and the reference's lines, all of them
    msgs = []
    neg = api.calculate_a_and_vara_rcpp(fMt, NA, g["S"], g["V"], -1.0, (L, n), g["ahat"], message=msgs.append)
    assert np.ravel(neg["a"]).tolist() == rec["scan_sentinel"][0].tolist() == [0.0]
    assert np.ravel(neg["vara"]).tolist() == rec["scan_sentinel"][1].tolist() == [0.0]
    assert len(rec["texts"]["scan_sentinel_messages"]) == 7 and msgs == rec["texts"]["scan_sentinel_messages"]
    # streamed: marker blocks of 512 through a resident budget too small for the file
    api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "%.6f" % (1.6 * 256 * 512 / 1e9))
    res = api.calculate_a_and_vara_rcpp(fMt, rec["sel_masked"], g["S"], g["V"], 8.0, (L, n), g["ahat"])
    if L >= 1000:
        assert api.last_stream_stats()["chunks"] > 1
    _check_scan(res, rec["a_masked_ld"], rec["vara_masked_ld"], idx=api.last_scan_argmax()[0], label="streamed")
    monkeypatch.delenv("EAGLE_HIP_MAX_RESIDENT_GB")
    api.drop_cache()
    # through a VIEW that drops nobody
    nd = api.ReshapeM_rcpp(fM, fMt, [], (n, L), view=True)
    assert nd == [n, L]
    res = api.calculate_a_and_vara_rcpp(fMt + "tmp", NA, g["S"], g["V"], 8.0, (L, n), g["ahat"])
    _check_scan(res, rec["a_na_ld"], rec["vara_na_ld"], idx=api.last_scan_argmax()[0], label="view")


@pytest.mark.parametrize("case", ALL_CASES)
def test_reduced_a(case, cases, api):
    g, geno, rec, _ = cases[case]
    n, L = g["M8"].shape
    ar = api.calculate_reduced_a_rcpp(geno["asciifileMt"], float(g["varG"]), g["P"], g["y"], 8.0, (n, L), NA)
    assert ar.shape == (L, 1)
    # test_gpu_parity.test_reduced_a's tolerance: rtol 1e-9, atol 1e-12 max|ref|
    np.testing.assert_allclose(ar.ravel(), rec["ar_ld"], rtol=1e-9, atol=1e-12 * np.abs(rec["ar_ld"]).max())
    msgs = []
    z = api.calculate_reduced_a_rcpp(geno["asciifileMt"], float(g["varG"]), g["P"], g["y"], 0.0, (n, L), NA, message=msgs.append)
    assert z.shape == rec["ar_sentinel"].shape == (1, 1) and z[0, 0] == rec["ar_sentinel"][0, 0] == 0.0
    assert msgs == rec["texts"]["ar_sentinel_messages"]
    api.drop_cache()


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_spectral_scan_and_scan_with_W(case, cases, api):
    """The scans that today are only checked against this library's other scan: spectral_prepare + spectral_scan and scan_with_W on
    K, X, y, varE, varG of the golden case -- the recorded a and vara come from the reference fed with the S, V, a_hat that
    host_model.scan_operands builds from the same quantities.  Tolerances of test_spectral_scan_matches_the_reference_shaped_scan."""
    g, geno, rec, _ = cases[case]
    n, L = g["M8"].shape
    K = g["MMt"] / g["MMt"].max() + 0.95 * np.eye(n)
    varE, varG, y = float(g["varE"]), float(g["varG"]), np.ravel(g["y"])
    ops = host_model.scan_operands(K, g["X"], y, varE, varG)
    np.testing.assert_allclose(ops["S"], g["S"], rtol=0, atol=1e-12 * np.abs(g["S"]).max())   # the operands the recording was fed with
    np.testing.assert_allclose(ops["V"], g["V"], rtol=0, atol=1e-12 * np.abs(g["V"]).max())
    a_ld, vara_ld = rec["a_na_ld"], rec["vara_na_ld"]
    idx_ref = _which_max(a_ld, vara_ld)[0]

    def check(res, label):
        np.testing.assert_allclose(np.ravel(res["a"]), a_ld, rtol=1e-8, atol=1e-10 * np.abs(a_ld).max(), err_msg=label)
        np.testing.assert_allclose(np.ravel(res["vara"]), vara_ld, rtol=9e-7, atol=1e-10 * np.abs(vara_ld).max(), err_msg=label)

    # The selected marker.  A marker that is constant over individuals has a = c 1'v and vara = c^2 1'W1, both zero in exact
    # arithmetic (X holds the intercept) and rounding noise of the operands' summation order in any real one: a^2 / vara there is
    # noise / noise, which neither the reference nor another order of the same sums can reproduce
    # (test_gpu_parity._selection_rests_on_noise).  Such markers -- |vara| of the reference below 1e-8 of its median, eight
    # orders above fp64 cancellation noise and eight below any real variance -- are left out of the arg-max; genoDemo has them.
    real = np.abs(vara_ld) > 1e-8 * np.median(np.abs(vara_ld))
    np.testing.assert_array_equal(real, g["M8"].max(axis=0) != g["M8"].min(axis=0))      # exactly the non-constant markers
    assert real[idx_ref - 1]

    def pick(res):
        with np.errstate(all="ignore"):
            tsq = np.where(real, np.ravel(res["a"]) ** 2 / np.ravel(res["vara"]), np.nan)
        return int(np.nanargmax(tsq)) + 1

    res = api.scan_with_W(geno["asciifileMt"], NA, varG ** 2 * ops["P"], varG * (ops["P"] @ y), 8.0, (L, n))
    check(res, "scan_with_W")
    assert pick(res) == idx_ref
    lam, U = np.linalg.eigh(K)
    api.spectral_prepare(geno["asciifileMt"], (L, n), U, 8.0)
    res = api.spectral_scan(lam, U.T @ g["X"], U.T @ y, varE, varG, L)
    check(res, "spectral_scan")
    assert pick(res) == idx_ref
    sel = rec["sel_masked"]
    res_m = api.spectral_scan(lam, U.T @ g["X"], U.T @ y, varE, varG, L, selected_loci=sel)
    np.testing.assert_allclose(np.ravel(res_m["a"]), rec["a_masked_ld"], rtol=1e-8, atol=1e-10 * np.abs(a_ld).max())
    np.testing.assert_allclose(np.ravel(res_m["vara"]), rec["vara_masked_ld"], rtol=9e-7, atol=1e-10 * np.abs(vara_ld).max())
    for s_ in sel.astype(int):   # (the spectral scan gives an exact 0 at constant markers too, so only the masked rows are asked for)
        assert res_m["a"][s_, 0] == 0.0 and res_m["vara"][s_, 0] == 0.0 and rec["vara_masked_ld"][s_] == 0.0
    api.drop_cache()


@pytest.mark.parametrize("case", ALL_CASES)
def test_converters_and_reshape_bytes(case, cases, api):
    g, geno, rec, d = cases[case]
    n, L = g["M8"].shape
    dig, texts = rec["digests"], rec["texts"]
    txt = refpin.write_text_table(str(d / "table.txt"), g["M8"])
    assert api.getRowColumn(txt) == [n, L]
    msgs = []
    assert api.createM_ASCII_rcpp(txt, str(d / "cM.ascii"), "text", 0, 1, 2, 8, [n, L], message=msgs.append)
    assert refpin.file_digest(d / "cM.ascii") == dig["createM_text"]
    assert refpin.scrub(msgs, d) == texts["createM_text_messages"]
    msgs = []
    api.createMt_ASCII_rcpp(str(d / "cM.ascii"), str(d / "cMt.ascii"), "text", 8, [n, L], message=msgs.append)
    assert refpin.file_digest(d / "cMt.ascii") == dig["createMt"]
    # the two lines that print a double are worded by R, which no build of src/*.cpp covers: every other line is compared
    plain = lambda ms: [m for m in refpin.scrub(ms, d) if "(gigabytes)" not in m]
    assert plain(msgs) == plain(texts["createMt_messages"])
    for label, na in refpin.na_sets(n).items():
        assert api.ReshapeM_rcpp(geno["asciifileM"], geno["asciifileMt"], na, (n, L)) == [n - len(na), L]
        assert refpin.file_digest(geno["asciifileM"] + "tmp") == dig["reshape_%s_M" % label], label
        assert refpin.file_digest(geno["asciifileMt"] + "tmp") == dig["reshape_%s_Mt" % label], label
    api.drop_cache()


def test_reference_data_pair_and_error_exits(cases, api, tmp_path):
    from eagleeverything_amd._lib import EagleError
    _, _, rec, _ = cases["geno_150x100"]
    dig, texts = rec["digests"], rec["texts"]
    ped, gtxt = os.path.join(refpin.GOLDEN, "geno_150x100.ped"), os.path.join(refpin.GOLDEN, "geno_150x100.txt")
    assert api.getRowColumn(ped) == list(rec["getRowColumn_ped"]) and api.getRowColumn(gtxt) == list(rec["getRowColumn_txt"])
    msgs = []
    assert api.createM_ASCII_rcpp(ped, str(tmp_path / "pM.ascii"), "PLINK", "-9", "-9", "-9", 8, [150, 206], message=msgs.append)
    assert refpin.file_digest(tmp_path / "pM.ascii") == dig["createM_plink"]
    assert msgs == texts["createM_plink_messages"]
    msgs = []
    api.createMt_ASCII_rcpp(str(tmp_path / "pM.ascii"), str(tmp_path / "pMt.ascii"), "PLINK", 8, [150, 100], message=msgs.append)
    assert refpin.file_digest(tmp_path / "pMt.ascii") == dig["createMt_plink"]
    plain = lambda ms: [m for m in refpin.scrub(ms, tmp_path) if "(gigabytes)" not in m]   # as in test_converters_and_reshape_bytes
    assert " File type:                   PLINK" in texts["createMt_plink_messages"]
    assert plain(msgs) == plain(texts["createMt_plink_messages"])
    assert api.createM_ASCII_rcpp(gtxt, str(tmp_path / "tM.ascii"), "text", 0, 1, 2, 8, [150, 100])
    assert refpin.file_digest(tmp_path / "tM.ascii") == dig["createM_goldentxt"]
    for name, (src, typ, AA, AB, BB, dims) in refpin.error_inputs(tmp_path).items():
        msgs = []
        out = tmp_path / (name + ".ascii")
        assert not api.createM_ASCII_rcpp(src, str(out), typ, AA, AB, BB, 8, dims, message=msgs.append), name
        assert refpin.scrub(msgs, tmp_path) == texts["error_%s_messages" % name], name
        assert refpin.file_digest(out) == dig["error_" + name], name
    with pytest.raises(EagleError) as e:
        api.ReadBlock(str(tmp_path / "absent"), 0, 3, 3)
    assert e.value.text.strip() == texts["stop_ReadBlock"].replace("<DIR>", str(tmp_path)).strip()
    with pytest.raises(EagleError) as e:
        api.getRowColumn(str(tmp_path / "absent"))
    assert e.value.text.strip() == texts["stop_getRowColumn"].replace("<DIR>", str(tmp_path)).strip()
    api.drop_cache()
