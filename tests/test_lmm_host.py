"""CPU: r_api.lmm_host, the numpy restatement of include/eagle_hip.h section 1d', against the 40-digit truth of tests/lmm_truth.py with
the bounds derived there (lmm_truth.bounds: the stop rule plus first-order rounding terms, no tuned number); golden entries recomputed
live; the planted special markers by their codes; max_iter = 0 against the P3D estimate from the dense P; and am.GWAS's bookkeeping
with the device calls replaced by their host restatements."""
import math

import numpy as np
import pytest

import lmm_truth as T
from eagleeverything_amd import am, host_model, r_api, rcpp_api

TOL = 1e-10
_ops = {}


def operands(name):
    if name not in _ops:
        _ops[name] = T.operands(name)
    return _ops[name]


def assert_meets_truth(name, method, stat, info, n):
    """Every clear marker: code 0 and theta, gamma, se, l within lmm_truth.bounds; at least 90 % of the panel's markers are clear."""
    t = T.golden(name)[method]
    clear = t["clear"] > 0.5
    assert clear.mean() >= 0.9, (name, method, clear.mean())
    for m in np.flatnonzero(clear):
        b = T.bounds(n, TOL, t, m)
        assert info[m, 0] == 0, (name, method, m, info[m])
        got = (math.log(stat[m, 2]), stat[m, 0], stat[m, 1], stat[m, 4])
        for what, g, k, bb in zip(("theta", "gamma", "se", "ll"), got, ("theta", "gamma", "se", "ll"), b):
            assert abs(g - t[k][m]) <= bb, (name, method, m, what, g, t[k][m], bb)
        assert stat[m, 3] > 0
    for m in np.flatnonzero(~clear & (t["code"] >= 2)):                     # a boundary optimum or a singular marker: the same code
        assert info[m, 0] == int(t["code"][m]), (name, method, m, info[m], t["code"][m])


@pytest.mark.parametrize("method", ["reml", "ml"])
@pytest.mark.parametrize("name", T.all_panels())
def test_host_meets_truth(name, method):
    lam, U, UtX, Uty, Z, th_r, th_m, Mt8, X, y = operands(name)
    stat, info = r_api.lmm_host(lam, UtX, Uty, Z, reml=method == "reml", theta0=th_r if method == "reml" else th_m, tol=TOL)
    assert stat.shape == (Mt8.shape[0], 5) and info.shape == (Mt8.shape[0], 2) and info.dtype == np.int32
    assert_meets_truth(name, method, stat, info, lam.size)


@pytest.mark.parametrize("name,m,method", [("n63", 1, "reml"), ("n65", 4, "ml"), ("c14", 0, "reml"), ("L129", 128, "ml"), ("n257", 0, "reml")])
def test_golden_entries_recomputed_live(name, m, method):
    """The stored truth is what lmm_truth computes today, to within the bounds it hands out (the eigenbasis is made again here)."""
    lam, U, UtX, Uty, Z, th_r, th_m, *_ = operands(name)
    t = T.golden(name)[method]
    live = T.marker_truth(lam, UtX, Uty, Z[m], th_r if method == "reml" else th_m, method == "reml")
    assert live["clear"] == t["clear"][m] and live["code"] == t["code"][m]
    b = T.bounds(lam.size, TOL, t, m)
    for k, bb in zip(("theta", "gamma", "se", "ll"), b):
        assert abs(live[k] - t[k][m]) <= bb, (k, live[k], t[k][m])
    for k in ("gp", "cond", "d_gamma", "d_se", "round_g", "round_gamma", "round_se", "round_ll"):
        assert live[k] == pytest.approx(t[k][m], rel=1e-6), k


def test_default_theta0_is_the_null_fit():
    lam, U, UtX, Uty, Z, th_r, th_m, *_ = operands("n64")
    for reml, th in ((True, th_r), (False, th_m)):
        a = r_api.lmm_host(lam, UtX, Uty, Z, reml=reml)
        b = r_api.lmm_host(lam, UtX, Uty, Z, reml=reml, theta0=th)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    for kw in (dict(tol=0.0), dict(tol=1.0), dict(max_iter=-1), dict(max_iter=1001)):
        with pytest.raises(ValueError):
            r_api.lmm_host(lam, UtX, Uty, Z, **kw)
    with pytest.raises(ValueError):
        r_api.lmm_host(lam, np.ones((lam.size, 15)), Uty, Z)


@pytest.mark.parametrize("reml", [True, False])
@pytest.mark.parametrize("kind", ["singular", "upper", "lower"])
def test_special_markers_by_code(kind, reml):
    lam, U, X, y, Mt8, rows, code = T.special(kind)
    UtX, Uty = U.T @ X, U.T @ y
    th = math.log((am.emma_REMLE_eig if reml else am.emma_MLE_eig)(lam, UtX, Uty)["delta"])
    stat, info = r_api.lmm_host(lam, UtX, Uty, Mt8.astype(np.float64) @ U, reml=reml, theta0=th)
    assert list(info[rows, 0]) == [code] * len(rows), info
    if code == 2:
        assert np.isnan(stat[rows]).all() and (info[2:, 0] != 2).all() and np.isfinite(stat[2:]).all()
    else:
        assert th == pytest.approx(10.0 if code == 4 else -10.0)          # the null fit is at the limit as well
        np.testing.assert_allclose(np.log(stat[rows, 2]), 10.0 if code == 4 else -10.0, rtol=1e-14)
        assert np.isfinite(stat[rows]).all()


@pytest.mark.parametrize("name", ["n65", "c4"])
def test_max_iter_zero_returns_the_p3d_estimate(name):
    """At max_iter = 0 the rule reports the values at theta0: with theta0 the null REML fit, gamma is the generalised least squares
    estimate under the null variance components, vg0 a / vara = m' P y / m' P m from the dense P of the original space.  Both routes
    solve with H = ve I + vg K and with D' H^-1 D: they agree to 8 (n + 16) 2^-53 (cond(H) + cond(D' H^-1 D)) relative."""
    lam, U, UtX, Uty, Z, th_r, th_m, Mt8, X, y = operands(name)
    n = lam.size
    r0 = am.emma_REMLE_eig(lam, UtX, Uty)
    stat, info = r_api.lmm_host(lam, UtX, Uty, Z, reml=True, theta0=math.log(r0["delta"]), max_iter=0)
    assert (info[:, 1] == 0).all() and set(info[:, 0]) <= {0, 1}
    np.testing.assert_allclose(stat[:, 2], r0["delta"], rtol=1e-14)
    K = (U * lam) @ U.T
    H = host_model.calculateH(K, r0["ve"], r0["vg"])
    P = host_model.calculateP(H, X)
    Hi = np.linalg.inv(H)
    for i in range(Mt8.shape[0]):
        m = Mt8[i].astype(np.float64)
        a, vara = r0["vg"] * (m @ P @ y), r0["vg"] ** 2 * (m @ P @ m)
        D = np.column_stack([X, m])
        bound = 8.0 * (n + 16) * T.U53 * (np.linalg.cond(H) + np.linalg.cond(D.T @ Hi @ D))
        assert abs(stat[i, 0] - r0["vg"] * a / vara) <= bound * abs(stat[i, 0]), (i, stat[i, 0], r0["vg"] * a / vara, bound)


class HostSpectral:
    """am.SpectralBackend without a device: K, its eigh and Z = Mt U on the host, counting what GWAS asks for."""
    device = 0

    def __init__(self, Mt8):
        self.Mt8, self.lam, self.U, self.calls = Mt8, None, None, 0

    @property
    def eig(self):
        return None if self.U is None else (self.lam, self.U)

    def calcMMt(self, geno, availmemGb, ncpu, selected_loci, quiet):
        self.calls += 1
        K = T.kinship(self.Mt8)
        self.lam, self.U = np.linalg.eigh(K)
        return K


@pytest.fixture
def host_gwas(monkeypatch):
    name = "L129"
    G, Mt8, X, y, _ = T.panel(name)
    be = HostSpectral(Mt8)
    ran = []

    def scan(lam, UtX, Uty, varE, varG, n_markers, selected_loci=np.nan, device=0):
        Z = Mt8.astype(np.float64) @ be.U
        d = 1.0 / (varE + varG * lam)
        A = UtX.T @ (d[:, None] * UtX)
        q = Z @ (d[:, None] * UtX)
        c1 = np.linalg.solve(A, UtX.T @ (d * Uty))
        a = varG * (Z @ (d * Uty) - q @ c1)
        vara = varG ** 2 * ((Z * Z) @ d - np.einsum("ij,ij->i", q, np.linalg.solve(A, q.T).T))
        return {"a": a.reshape(-1, 1), "vara": vara.reshape(-1, 1)}

    def lmm(lam, UtX, Uty, reml=True, theta0=0.0, tol=1e-10, max_iter=50, idx=None, n_markers=None, device=0):
        rows = np.arange(Mt8.shape[0]) if idx is None else np.asarray(idx)
        ran.append(rows.copy())
        return r_api.lmm_host(lam, UtX, Uty, Mt8[rows].astype(np.float64) @ be.U, reml=reml, theta0=theta0, tol=tol, max_iter=max_iter)

    monkeypatch.setattr(rcpp_api, "spectral_scan", scan)
    monkeypatch.setattr(rcpp_api, "spectral_lmm", lmm)
    monkeypatch.setattr(rcpp_api, "spectral_holds", lambda f, U, device=0: be.U is not None and U is be.U)
    geno = {"asciifileM": "M", "asciifileMt": "Mt", "dim_of_ascii_M": [Mt8.shape[1], Mt8.shape[0]]}
    return Mt8, X, y, geno, be, ran, scan


def test_gwas_null_fit_and_score_are_emma_and_the_scan(host_gwas):
    Mt8, X, y, geno, be, ran, scan = host_gwas
    L, n = Mt8.shape
    out = r_api.GWAS(y, X, geno, backend=be)
    assert be.calls == 1 and out["n_used"] == n and out["method"] == "reml" and len(out["indxNA"]) == 0
    lam, U = be.eig
    UtX, Uty = U.T @ X, U.T @ y
    r0 = am.emma_REMLE_eig(lam, UtX, Uty)
    assert out["null"] == {"delta": r0["delta"], "vg": r0["vg"], "ve": r0["ve"], "ll": r0["REML"]}
    s = scan(lam, UtX, Uty, r0["ve"], r0["vg"], L)
    a, vara = s["a"].ravel(), s["vara"].ravel()
    np.testing.assert_array_equal(out["score"], a * a / vara)
    np.testing.assert_array_equal(out["beta_p3d"], r0["vg"] * a / vara)
    from scipy.special import chdtrc, fdtrc
    from scipy.stats import chi2
    np.testing.assert_array_equal(out["p_score"], chdtrc(1.0, out["score"]))
    assert out["lambda_gc"] == pytest.approx(np.median(out["score"]) / chi2.ppf(0.5, 1), rel=1e-12)
    stat, info = r_api.lmm_host(lam, UtX, Uty, Mt8.astype(np.float64) @ U, theta0=math.log(r0["delta"]))
    for j, k in enumerate(("beta", "se", "delta", "vg", "ll")):
        np.testing.assert_array_equal(out[k], stat[:, j])
    np.testing.assert_array_equal(out["ve"], stat[:, 2] * stat[:, 3])
    np.testing.assert_array_equal(out["code"], info[:, 0])
    np.testing.assert_array_equal(out["iterations"], info[:, 1])
    np.testing.assert_array_equal(out["stat"], (stat[:, 0] / stat[:, 1]) ** 2)
    np.testing.assert_array_equal(out["p"], fdtrc(1.0, n - X.shape[1] - 1.0, out["stat"]))
    # a second call on the same backend rebuilds nothing; exact="none" and p_exact
    none = am.GWAS(y, X, geno, exact="none", backend=be)
    assert be.calls == 1 and len(ran) == 1
    assert all(np.isnan(none[k]).all() for k in am._GWAS_EXACT) and (none["code"] == -1).all() and (none["iterations"] == 0).all()
    np.testing.assert_array_equal(none["score"], out["score"])
    scr = am.GWAS(y, X, geno, p_exact=0.05, backend=be, map=["snp%d" % i for i in range(L)])
    hit = np.flatnonzero(out["p_score"] < 0.05)
    assert 0 < hit.size < L and np.array_equal(ran[-1], hit) and scr["names"][3] == "snp3"
    for k in am._GWAS_EXACT + ("code", "iterations"):
        np.testing.assert_array_equal(scr[k][hit], out[k][hit])
    rest = np.setdiff1d(np.arange(L), hit)
    assert np.isnan(scr["p"][rest]).all() and (scr["code"][rest] == -1).all()


def test_gwas_ml_is_a_likelihood_ratio_test_and_refusals(host_gwas):
    Mt8, X, y, geno, be, ran, scan = host_gwas
    out = am.GWAS(y, X, geno, method="ml", backend=be)
    lam, U = be.eig
    UtX, Uty = U.T @ X, U.T @ y
    m0 = am.emma_MLE_eig(lam, UtX, Uty)
    assert out["null"]["ll"] == m0["ML"] and out["null"]["delta"] == m0["delta"] and out["null_reml"]["delta"] == am.emma_REMLE_eig(lam, UtX, Uty)["delta"]
    stat, info = r_api.lmm_host(lam, UtX, Uty, Mt8.astype(np.float64) @ U, reml=False, theta0=math.log(m0["delta"]))
    from scipy.special import chdtrc
    np.testing.assert_array_equal(out["stat"], np.maximum(2.0 * (stat[:, 4] - m0["ML"]), 0.0))
    np.testing.assert_array_equal(out["p"], chdtrc(1.0, out["stat"]))
    assert (out["stat"][info[:, 0] == 0] >= 0).all()
    # the null model is nested in every marker's: at the null's own delta the marker model's likelihood is already no smaller
    assert (stat[info[:, 0] == 0, 4] >= m0["ML"] - 1e-9).all()
    with pytest.raises(NotImplementedError, match="Zmat"):
        am.GWAS(y, X, geno, backend=be, Zmat=np.eye(3))
    for kw in (dict(exact="some"), dict(method="wald"), dict(p_exact=0.0), dict(p_exact=1.5), dict(map=["a"])):
        with pytest.raises(ValueError):
            am.GWAS(y, X, geno, backend=be, **kw)
    with pytest.raises(ValueError):
        am.GWAS(y, np.ones((y.size, 15)), geno, backend=be)
    with pytest.raises(TypeError):
        am.GWAS(y, X, geno, backend=object())
