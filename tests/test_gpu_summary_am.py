"""SummaryAM on the GPU path (r_api.SummaryAM, am.SummaryAM_traits): calcMMt, extract_geno and the NA reshape through the HIP
library, eigh on host LAPACK or on the device (algebra="device"), the marker columns of U^T F from the resident Z after AM_traits.
Yardstick: the literal restatement of summary_am.R in test_summary_am_host.py, on the oracle's MM^T."""
import numpy as np
import pytest

from eagleeverything_amd import am, host_model, r_api, rcpp_api, synth

from test_summary_am_host import (CountingLA, assert_matches_straight, assert_same_tables, oracle_K, planted,
                                  straight_summary)

pytestmark = pytest.mark.gpu


def _msel(Mt8, picks, keep=None):
    M = Mt8[np.array(picks) - 1].T.astype(float)
    return M if keep is None else M[keep]


def test_summary_am_hip_matches_straight_restatement(oracle, golden, tmp_path):
    g = golden("genoDemo_150x4998")
    Mt8, y = planted(g)
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    res = am.AM(y, g["X"], geno, maxit=8)
    assert len(res["selected_loci"]) >= 3
    got = r_api.SummaryAM(res, y, g["X"], geno)
    assert_matches_straight(got, straight_summary(y, g["X"], _msel(Mt8, res["selected_loci"]), oracle_K(oracle, geno)))
    assert got["pvalue"]["effects"] == ["intercept", "X2", "X3"] + ["M%d" % j for j in res["selected_loci"]]


def test_summary_am_hip_with_na_rows_uses_the_view_reshape(oracle, golden, tmp_path):
    g = golden("genoDemo_150x4998")
    Mt8, y = planted(g, seed=2)
    y[[7, 64, 101]] = np.nan
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    res = am.AM(y, g["X"], geno, maxit=8)
    assert list(res["indxNA"]) == [102, 65, 8] and len(res["selected_loci"]) >= 3
    got = r_api.SummaryAM(res, y, g["X"], geno)
    keep = ~np.isnan(y)
    K = oracle_K(oracle, am.reshape_geno(geno, res["indxNA"]))                       # the oracle reads rewritten files
    assert_matches_straight(got, straight_summary(y[keep], g["X"][keep], _msel(Mt8, res["selected_loci"], keep), K))


def test_summary_am_device_algebra_matches_straight_restatement(oracle, golden, tmp_path):
    g = golden("genoDemo_150x4998")
    Mt8, y = planted(g)
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    res = am.AM(y, g["X"], geno, maxit=8)
    host_model.set_algebra("device")
    try:
        got = r_api.SummaryAM(res, y, g["X"], geno)
    finally:
        host_model.set_algebra("host")
    assert_matches_straight(got, straight_summary(y, g["X"], _msel(Mt8, res["selected_loci"]), oracle_K(oracle, geno)))


def test_summary_am_with_eig_from_spectral_backend(oracle, golden, tmp_path, monkeypatch):
    g = golden("genoDemo_150x4998")
    Mt8, y = planted(g)
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    ref = am.AM(y, g["X"], geno, maxit=8)
    spec = am.SpectralBackend()
    assert spec.eig is None
    res = am.AM(y, g["X"], geno, maxit=8, backend=spec)
    assert res["all_picks"] == ref["all_picks"] and res["selected_loci"] == ref["selected_loci"]
    la = CountingLA(host_model.algebra())
    monkeypatch.setattr(host_model, "_la", la)
    got = r_api.SummaryAM(res, y, g["X"], geno, eig=spec.eig)
    assert la.eighs == 0
    assert_matches_straight(got, straight_summary(y, g["X"], _msel(Mt8, res["selected_loci"]), oracle_K(oracle, geno)))


def test_summary_am_traits_z_rows_equal_host_u(golden, tmp_path, monkeypatch):
    g = golden("genoDemo_150x4998")
    Mt8, y = planted(g)
    rng = np.random.default_rng(5)
    M = Mt8.T.astype(float)
    Y = np.column_stack([y] + [M[:, qs] @ b + 0.6 * rng.standard_normal(150)
                               for qs, b in (([100, 2000, 3500], [1.2, 1.0, -1.1]), ([700, 2900, 4600], [-1.4, 1.0, 0.9]))])
    Y[[4, 40], 1] = np.nan
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    res = am.AM_traits(Y, g["X"], geno, maxit=6)
    assert all(r["selected_loci"] for r in res)
    calls = []
    rows = rcpp_api.spectral_rows
    monkeypatch.setattr(rcpp_api, "spectral_rows", lambda idx, device=0: calls.append(len(idx)) or rows(idx, device=device))
    z = am.SummaryAM_traits(res, Y, g["X"], geno)
    assert calls == [len({j for r in res for j in r["selected_loci"]})]          # the Z-rows path ran, once for all traits
    monkeypatch.setattr(rcpp_api, "spectral_holds", lambda *a, **k: False)
    h = am.SummaryAM_traits(res, Y, g["X"], geno)
    assert len(calls) == 1
    for a, b in zip(z, h):
        assert_same_tables(a, b, rtol=1e-10)
    for t in range(Y.shape[1]):                                                    # and trait t alone
        yt = Y[:, t].copy()
        yt[np.isnan(Y).any(axis=1)] = np.nan
        assert_same_tables(z[t], r_api.SummaryAM(res[t], yt, g["X"], geno), rtol=1e-10)
    rcpp_api.drop_cache()


def test_summary_am_at_2000_by_50000(tmp_path):
    n, L = 2000, 50000
    Mt8 = synth.genotypes_marker_major(n, L, seed=21)
    y, qtl = synth.trait(Mt8, nqtl=6, beta=0.35, seed=4)
    X = np.column_stack([np.ones(n), np.random.default_rng(8).standard_normal(n)])
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    spec = am.SpectralBackend()
    res = am.AM(y, X, geno, maxit=8, backend=spec)
    assert len(res["selected_loci"]) >= 3
    with_eig = r_api.SummaryAM(res, y, X, geno, eig=spec.eig)
    fresh = r_api.SummaryAM(res, y, X, geno)
    assert_same_tables(with_eig, fresh, rtol=1e-8)
    K = r_api.calcMMt(geno, 8, 1, np.array([np.nan]), True)
    assert_matches_straight(with_eig, straight_summary(y, X, _msel(Mt8, res["selected_loci"]), K))
    rcpp_api.drop_cache()
