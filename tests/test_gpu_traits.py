"""Many traits in one pass over Z (eagle_spectral_scan_traits, eagle_spectral_rows; header section 1d) and AM_traits on an MI355X.

The batched scan must give what one eagle_spectral_scan per trait gives on the same prepare -- over several column groups, ragged
shapes and a context of two devices -- and AM_traits must pick, trait by trait, what AM() with the SpectralBackend picks."""
import numpy as np
import pytest

from eagleeverything_amd import am, rcpp_api, synth
from eagleeverything_amd._lib import EagleError

pytestmark = pytest.mark.gpu
P_CHOICES = (1, 4, 20, 31)


def _panel(tmp_path, n, L, seed=5):
    Mt8 = synth.genotypes_marker_major(n, L, seed=seed)
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    G = Mt8.astype(np.float64)
    K = G.T @ G
    K = K / K.max() + 0.95 * np.eye(n)
    lam, U = np.linalg.eigh(K)
    return Mt8, geno, K, lam, U


def _traits(Mt8, T, seed):
    """T traits with p_t cycling through P_CHOICES; X_t = [1, one marker of the panel (in the model), random covariates]."""
    L, n = Mt8.shape
    rng = np.random.default_rng(seed)
    Xs, inm = [], []
    for t in range(T):
        p = P_CHOICES[t % len(P_CHOICES)]
        cols = [np.ones(n)]
        if p >= 2:
            j = int(rng.integers(L))
            inm.append((t, j))
            cols.append(Mt8[j].astype(np.float64))
        cols += [rng.standard_normal(n) for _ in range(p - len(cols))]
        Xs.append(np.column_stack(cols))
    Y = np.column_stack([Mt8[int(rng.integers(L))] * 0.8 + rng.standard_normal(n) for _ in range(T)])
    vE = rng.uniform(0.3, 1.5, T)
    vG = rng.uniform(0.2, 1.2, T)
    return Xs, Y, vE, vG, inm


def _compare_with_single(lam, U, K, Mt8, Xs, Y, vE, vG, inm, device=0, rows=None):
    L = Mt8.shape[0]
    T = Y.shape[1]
    UtX = [U.T @ X for X in Xs]
    res = rcpp_api.spectral_scan_traits(lam, UtX, U.T @ Y, vE, vG, L, full=True, device=device)
    assert res["a"].shape == (L, T)
    for t in range(T):
        one = rcpp_api.spectral_scan(lam, UtX[t], U.T @ Y[:, t], vE[t], vG[t], L, device=device)
        a1, v1 = one["a"].ravel(), one["vara"].ravel()
        a, v = res["a"][:, t], res["vara"][:, t]
        np.testing.assert_allclose(a, a1, rtol=1e-12, atol=1e-12 * np.abs(a1).max())
        np.testing.assert_allclose(v, v1, rtol=1e-10, atol=1e-12 * np.abs(v1).max())
        np.testing.assert_array_equal(a1 == 0.0, a == 0.0)
        with np.errstate(all="ignore"):
            tsq1 = a1 * a1 / v1
        assert res["index"][t] == int(np.nanargmax(tsq1)) + 1
        assert res["tsqmax"][t] == pytest.approx(np.nanmax(tsq1), rel=1e-10)
    for t, j in inm:
        assert res["a"][j, t] == 0.0 and res["vara"][j, t] == 0.0
    # the fp64 definition on a row sample: a_i = varG m_i^T P y, vara_i = varG^2 m_i^T P m_i
    rows = np.r_[0:20, L // 2:L // 2 + 20, L - 20:L] if rows is None else rows
    M = Mt8[rows].astype(np.float64)
    n = K.shape[0]
    for t in (0, T - 1):
        H = vE[t] * np.eye(n) + vG[t] * K
        Hi = np.linalg.inv(H)
        X = Xs[t]
        P = Hi - Hi @ X @ np.linalg.solve(X.T @ Hi @ X, X.T @ Hi)
        keep = ~np.isin(rows, [j for tt, j in inm if tt == t])
        np.testing.assert_allclose(res["a"][rows[keep], t], vG[t] * (M[keep] @ (P @ Y[:, t])), rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(res["vara"][rows[keep], t], vG[t] ** 2 * np.einsum("ij,jk,ik->i", M[keep], P, M[keep]), rtol=1e-8)
    return res


@pytest.mark.parametrize("T", [1, 3, 17])
def test_batched_scan_equals_single_scans(tmp_path, T):
    Mt8, geno, K, lam, U = _panel(tmp_path, 300, 3000)
    L, n = Mt8.shape
    rcpp_api.spectral_prepare(geno["asciifileMt"], (L, n), U, 8.0)
    Xs, Y, vE, vG, inm = _traits(Mt8, T, seed=T)
    if T == 17:
        assert rcpp_api.spectral_traits_passes([X.shape[1] for X in Xs]) > 1
    res = _compare_with_single(lam, U, K, Mt8, Xs, Y, vE, vG, inm)
    # full=False: only the arg-max comes back, the same one
    lean = rcpp_api.spectral_scan_traits(lam, [U.T @ X for X in Xs], U.T @ Y, vE, vG, L)
    np.testing.assert_array_equal(lean["index"], res["index"])
    np.testing.assert_array_equal(lean["tsqmax"], res["tsqmax"])
    rcpp_api.drop_cache()


@pytest.mark.parametrize("n,L", [(1003, 5000), (1003, 200)])
def test_batched_scan_ragged_shapes(tmp_path, n, L):
    Mt8, geno, K, lam, U = _panel(tmp_path, n, L, seed=8)
    rcpp_api.spectral_prepare(geno["asciifileMt"], (L, n), U, 8.0)
    Xs, Y, vE, vG, inm = _traits(Mt8, 5, seed=n + L)
    _compare_with_single(lam, U, K, Mt8, Xs, Y, vE, vG, inm, rows=np.r_[0:10, L - 10:L])
    rcpp_api.drop_cache()


def test_batched_scan_two_contexts_on_one_card(tmp_path):
    n, L = 300, 3000
    Mt8 = synth.genotypes_marker_major(n, L, seed=6)
    lo, hi = 100, 2900                        # the device split of 3000 markers over two contexts is at 1536
    Mt8[hi] = Mt8[lo]
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    G = Mt8.astype(np.float64)
    K = G.T @ G
    K = K / K.max() + 0.95 * np.eye(n)
    lam, U = np.linalg.eigh(K)
    rng = np.random.default_rng(2)
    Xs, Y, vE, vG, _ = _traits(Mt8, 6, seed=21)
    Y[:, 0] = 3.0 * G[lo] + 0.3 * rng.standard_normal(n)        # planted on the duplicated marker
    Xs[0] = np.ones((n, 1))
    out = {}
    for dev in (0, (0, 0)):
        rcpp_api.spectral_prepare(geno["asciifileMt"], (L, n), U, 8.0, device=dev)
        out[dev] = rcpp_api.spectral_scan_traits(lam, [U.T @ X for X in Xs], U.T @ Y, vE, vG, L, full=True, device=dev)
        rcpp_api.drop_cache(device=dev)
    for k in ("a", "vara", "index", "tsqmax"):
        np.testing.assert_array_equal(out[0][k], out[(0, 0)][k], err_msg=k)
    assert out[0]["a"][lo, 0] == out[0]["a"][hi, 0] and out[0]["vara"][lo, 0] == out[0]["vara"][hi, 0]
    assert out[(0, 0)]["index"][0] == lo + 1


def test_spectral_rows_are_Ut_m(tmp_path):
    Mt8, geno, K, lam, U = _panel(tmp_path, 1003, 700, seed=3)
    L, n = Mt8.shape
    for dev in (0, (0, 0)):
        rcpp_api.spectral_prepare(geno["asciifileMt"], (L, n), U, 8.0, device=dev)
        idx = np.array([0, 5, 255, 256, 511, L - 1, 5])
        Z = rcpp_api.spectral_rows(idx, device=dev)
        assert Z.shape == (n, idx.size)
        ref = U.T @ Mt8[idx].T.astype(np.float64)
        bound = np.abs(Mt8[idx]).sum(axis=1).astype(np.float64) * 2.0 ** (0 + 1 - 48) + 1e-13
        assert np.all(np.abs(Z - ref) <= bound[None, :])
        rcpp_api.drop_cache(device=dev)


def _demo_traits(golden):
    g = golden("genoDemo_150x4998")
    Mt8 = np.ascontiguousarray(g["M8"].T)
    traits = [g["y"]]
    for nqtl, beta, seed in ((2, 1.0, 3), (3, 0.8, 5), (4, 0.7, 9)):
        traits.append(synth.trait(Mt8, nqtl=nqtl, beta=beta, seed=seed)[0])
    Y = np.column_stack(traits)
    Y[[4, 40, 77, 120], 2] = np.nan
    return g, Mt8, Y


def test_am_traits_equals_am_spectral(golden, tmp_path):
    g, Mt8, Y = _demo_traits(golden)
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    maxit = 6
    res = am.AM_traits(Y, g["X"], geno, maxit=maxit)
    union = np.isnan(Y).any(axis=1)
    for t in range(Y.shape[1]):
        y = Y[:, t].copy()
        y[union] = np.nan
        ref = am.AM(y, g["X"], geno, maxit=maxit, backend=am.SpectralBackend())
        assert res[t]["all_picks"] == ref["all_picks"] and res[t]["selected_loci"] == ref["selected_loci"], t
        np.testing.assert_allclose(res[t]["extBIC_trace"], ref["extBIC_trace"], rtol=1e-8)
        np.testing.assert_allclose([res[t]["ve"], res[t]["vg"]], [ref["ve"], ref["vg"]], rtol=1e-6)
        np.testing.assert_array_equal(res[t]["indxNA"], ref["indxNA"])
        assert res[t]["dim_of_ascii_M"] == ref["dim_of_ascii_M"]
    # one trait: the same run as AM() with the SpectralBackend
    one = am.AM_traits(g["y"], g["X"], geno, maxit=maxit)[0]
    ref = am.AM(g["y"], g["X"], geno, maxit=maxit, backend=am.SpectralBackend())
    assert one["all_picks"] == ref["all_picks"] and one["selected_loci"] == ref["selected_loci"]
    np.testing.assert_allclose(one["extBIC_trace"], ref["extBIC_trace"], rtol=1e-8)
    assert len(ref["all_picks"]) >= 2


def test_scan_traits_argument_errors_leave_the_context_usable(tmp_path):
    rcpp_api.close_all()
    Mt8, geno, K, lam, U = _panel(tmp_path, 300, 1000, seed=4)
    L, n = Mt8.shape
    Xs, Y, vE, vG, _ = _traits(Mt8, 2, seed=1)
    UtX, UtY = [U.T @ X for X in Xs], U.T @ Y

    def err(msg, *args, **kw):
        with pytest.raises(EagleError) as e:
            rcpp_api.spectral_scan_traits(*args, **kw)
        assert e.value.code == -3 and msg in e.value.text, e.value.text

    err("has not run", lam, UtX, UtY, vE, vG, L)
    with pytest.raises(EagleError, match="has not run"):
        rcpp_api.spectral_rows([0])
    rcpp_api.spectral_prepare(geno["asciifileMt"], (L, n), U, 8.0)
    err("1 <= p <= 31", lam, [UtX[0], np.zeros((n, 0))], UtY, vE, vG, L)
    err("1 <= p <= 31", lam, [UtX[0], np.ones((n, 32))], UtY, vE, vG, L)
    err("T >= 1", lam, [], np.zeros((n, 0)), [], [], L)
    err("must be positive", lam, UtX, UtY, [vE[0], -10.0], [vG[0], 1e-3], L)
    err("not positive definite", lam, [UtX[0], np.column_stack([UtX[1], np.zeros(n)])], UtY, vE, vG, L)
    with pytest.raises(EagleError, match="out of range"):
        rcpp_api.spectral_rows([L])
    res = rcpp_api.spectral_scan_traits(lam, UtX, UtY, vE, vG, L, full=True)
    for t in range(2):
        one = rcpp_api.spectral_scan(lam, UtX[t], UtY[:, t], vE[t], vG[t], L)
        np.testing.assert_allclose(res["a"][:, t], one["a"].ravel(), rtol=1e-12, atol=1e-12 * np.abs(one["a"]).max())
    rcpp_api.drop_cache()
