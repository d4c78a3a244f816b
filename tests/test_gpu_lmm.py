"""The exact mixed-model test on an MI355X (eagle_spectral_lmm, k_lmm_exact; include/eagle_hip.h section 1d'): the three sweeps of
tests/lmm_truth.py for both methods against the 40-digit truth with the bounds derived there, the special markers by their codes, bit
equality of all markers / an index list in reversed order / a second call, the argument errors that need a prepared context, and
am.GWAS end to end.

The sweeps prepare Z on the fp64 MFMA (set_scan_mode(0)): the truth's bounds carry fp64 rounding of the operands, n 2^-53, and the
default digit-slice build of Z is documented to n 2^-47.  GWAS end to end runs on the default build."""
import math

import numpy as np
import pytest

import lmm_truth as T
from eagleeverything_amd import am, r_api, rcpp_api, synth
from eagleeverything_amd._lib import EagleError
from test_lmm_host import TOL, assert_meets_truth, operands

pytestmark = pytest.mark.gpu


def _prepare(tmp_path, Mt8, U, mode=0):
    L, n = Mt8.shape
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    rcpp_api.set_scan_mode(mode)
    try:
        rcpp_api.spectral_prepare(geno["asciifileMt"], (L, n), U, 8.0)
    finally:
        rcpp_api.set_scan_mode(1)
    return geno


@pytest.mark.parametrize("name", T.all_panels())
def test_device_meets_truth(tmp_path, name):
    lam, U, UtX, Uty, Z, th_r, th_m, Mt8, X, y = operands(name)
    L, n = Mt8.shape
    _prepare(tmp_path, Mt8, U)
    for method, th in (("reml", th_r), ("ml", th_m)):
        stat, info = rcpp_api.spectral_lmm(lam, UtX, Uty, reml=method == "reml", theta0=th, tol=TOL, n_markers=L)
        assert stat.shape == (L, 5) and info.shape == (L, 2)
        assert_meets_truth(name, method, stat, info, n)
        # all markers == an index list in reversed order == a second call
        rev = np.arange(L)[::-1].copy()
        s2, i2 = rcpp_api.spectral_lmm(lam, UtX, Uty, reml=method == "reml", theta0=th, tol=TOL, idx=rev)
        s3, i3 = rcpp_api.spectral_lmm(lam, UtX, Uty, reml=method == "reml", theta0=th, tol=TOL, n_markers=L)
        assert stat[rev].tobytes() == s2.tobytes() and np.array_equal(info[rev], i2)
        assert stat.tobytes() == s3.tobytes() and np.array_equal(info, i3)
    rcpp_api.drop_cache()


@pytest.mark.parametrize("kind", ["singular", "upper", "lower"])
def test_special_markers_by_code(tmp_path, kind):
    lam, U, X, y, Mt8, rows, code = T.special(kind)
    UtX, Uty = U.T @ X, U.T @ y
    _prepare(tmp_path, Mt8, U)
    for reml, fit in ((True, am.emma_REMLE_eig), (False, am.emma_MLE_eig)):
        th = math.log(fit(lam, UtX, Uty)["delta"])
        stat, info = rcpp_api.spectral_lmm(lam, UtX, Uty, reml=reml, theta0=th, n_markers=Mt8.shape[0])
        assert list(info[rows, 0]) == [code] * len(rows), info
        if code == 2:
            assert np.isnan(stat[rows]).all() and (info[2:, 0] != 2).all() and np.isfinite(stat[2:]).all()
        else:
            np.testing.assert_allclose(np.log(stat[rows, 2]), 10.0 if code == 4 else -10.0, rtol=1e-14)
            assert np.isfinite(stat[rows]).all()
        hs, hi = r_api.lmm_host(lam, UtX, Uty, Mt8.astype(np.float64) @ U, reml=reml, theta0=th)
        np.testing.assert_array_equal(info, hi)
    rcpp_api.drop_cache()


def test_max_iter_zero_and_argument_errors(tmp_path):
    lam, U, UtX, Uty, Z, th_r, th_m, Mt8, X, y = operands("n65")
    L, n = Mt8.shape
    rcpp_api.close_all()                                                   # a context without a prepare
    (tmp_path / "s").mkdir()
    (tmp_path / "t").mkdir()
    with pytest.raises(EagleError) as e:
        rcpp_api.spectral_lmm(lam, UtX, Uty, n_markers=L)
    assert e.value.code == -3 and "eagle_spectral_prepare has not run" in e.value.text
    _prepare(tmp_path, Mt8, U)
    stat, info = rcpp_api.spectral_lmm(lam, UtX, Uty, theta0=th_r, max_iter=0, n_markers=L)
    hs, hi = r_api.lmm_host(lam, UtX, Uty, Z, theta0=th_r, max_iter=0)
    assert (info[:, 1] == 0).all() and np.array_equal(info, hi)
    np.testing.assert_allclose(stat, hs, rtol=1e-9)
    np.testing.assert_allclose(stat[:, 2], math.exp(th_r), rtol=1e-14)
    empty = rcpp_api.spectral_lmm(lam, UtX, Uty, idx=[])
    assert empty[0].shape == (0, 5) and empty[1].shape == (0, 2)
    bad_lam = lam.copy()
    bad_lam[5] = -1.0
    for kw, text in ((dict(idx=[0, L]), "marker index out of range"), (dict(lam=bad_lam), "lambda_k + e^-10 must be positive"),
                     (dict(lam=lam[:16], UtX=np.ones((16, 14)), Uty=Uty[:16]), "n <= c + 2")):
        args = dict(lam=lam, UtX=UtX, Uty=Uty, n_markers=L)
        args.update(kw)
        if "n <= c + 2" == text:                                           # the resident Z decides n: prepare a panel of 16 individuals
            rcpp_api.spectral_prepare(synth.write_geno_pair(str(tmp_path / "s"), Mt8[:, :16].copy())["asciifileMt"], (L, 16), np.eye(16), 8.0)
        with pytest.raises(EagleError) as e:
            rcpp_api.spectral_lmm(**args)
        assert e.value.code == -3 and text in e.value.text, (text, e.value.text)
    rcpp_api.spectral_prepare(synth.write_geno_pair(str(tmp_path / "t"), Mt8)["asciifileMt"], (L, n), U, 8.0, device=(0, 0))
    with pytest.raises(EagleError) as e:
        rcpp_api.spectral_lmm(lam, UtX, Uty, n_markers=L, device=(0, 0))
    assert e.value.code == -3 and "multi-device" in e.value.text
    rcpp_api.close_all()


def test_gwas_end_to_end(golden, tmp_path, monkeypatch):
    g = golden("synth_203x1531")
    Mt8 = np.ascontiguousarray(g["M8"].T)
    L, n = Mt8.shape
    rng = np.random.default_rng(3)
    X = np.column_stack([np.ones(n), rng.standard_normal(n)])
    qtl = 700
    # a polygenic part on every marker and noise in the proportion that puts the null fit's delta inside (-10, 10), one planted marker
    y = X @ [1.0, 0.3] + 1.5 * Mt8[qtl].astype(np.float64) + 0.06 * (Mt8.astype(np.float64).T @ rng.standard_normal(L)) \
        + 1.5 * rng.standard_normal(n)
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    prepares = []
    real = rcpp_api.spectral_prepare
    monkeypatch.setattr(rcpp_api, "spectral_prepare", lambda *a, **k: (prepares.append(1), real(*a, **k))[1])
    be = am.SpectralBackend()
    res = am.AM(y, X, geno, maxit=4, backend=be)
    assert len(prepares) == 1 and qtl + 1 in res["all_picks"]
    out = r_api.GWAS(y, X, geno, backend=be, map=["m%d" % i for i in range(L)])
    assert len(prepares) == 1                                              # the resident Z of AM() is reused
    ok = out["code"] == 0
    assert ok.mean() > 0.9 and set(out["code"]) <= {0, 3, 4} and out["n_used"] == n and out["names"][qtl] == "m%d" % qtl
    for k in am._GWAS_EXACT:
        assert np.isfinite(out[k][ok]).all(), k
    assert int(np.argmin(out["p"])) == qtl and int(np.argmax(out["score"])) == qtl
    assert 0.5 < out["lambda_gc"] < 2.0
    lam, U = be.eig
    r0 = am.emma_REMLE_eig(lam, U.T @ X, U.T @ y)
    assert out["null"]["delta"] == r0["delta"] and out["null"]["vg"] == r0["vg"]
    hs, hi = r_api.lmm_host(lam, U.T @ X, U.T @ y, rcpp_api.spectral_rows(np.arange(0, L, 50)).T, theta0=math.log(r0["delta"]))
    np.testing.assert_array_equal(out["code"][::50], hi[:, 0])
    np.testing.assert_allclose(out["beta"][::50][hi[:, 0] == 0], hs[hi[:, 0] == 0, 0], rtol=1e-7, atol=1e-10)
    none = am.GWAS(y, X, geno, exact="none", backend=be)
    assert all(np.isnan(none[k]).all() for k in am._GWAS_EXACT) and (none["code"] == -1).all()
    np.testing.assert_array_equal(none["score"], out["score"])
    scr = am.GWAS(y, X, geno, p_exact=1e-2, backend=be)
    hit = out["p_score"] < 1e-2
    assert 0 < hit.sum() < L and np.array_equal(scr["code"] >= 0, hit)
    for k in am._GWAS_EXACT + ("code", "iterations"):
        assert scr[k][hit].tobytes() == out[k][hit].tobytes(), k
        assert k in ("code", "iterations") or np.isnan(scr[k][~hit]).all()
    ml = am.GWAS(y, X, geno, method="ml", backend=be)
    assert int(np.argmin(ml["p"])) == qtl and len(prepares) == 1
    yna = y.copy()
    yna[[3, 77]] = np.nan
    na = am.GWAS(yna, X, geno, exact="none")                               # a fresh backend, a VIEW reshape
    assert na["n_used"] == n - 2 and list(na["indxNA"]) == [78, 4] and int(np.argmax(na["score"])) == qtl
    rcpp_api.drop_cache()
