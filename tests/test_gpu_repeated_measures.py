"""Repeated measures on the device (AM(Zmat=)): the reference-shaped scan with operands from Z^T P Z and
the spectral scan through eagle_spectral_scan_weights, against the dense oracle of tests/test_repeated_measures_host.py (n_obs x
n_obs matrices, the literal EMMA route), and by reduction to the cases the model without Z defines."""
import ctypes as C

import numpy as np
import pytest

from eagleeverything_amd import _lib, am, host_model, r_api, rcpp_api, synth
from test_repeated_measures_host import REL, dense_AM, dense_Z, dense_scan, drop_empty, kinship, rm_fixture, tsq_argmax

pytestmark = pytest.mark.gpu
NA = np.nan


def _files(tmp_path, M, stem=""):
    """M: individuals x markers, values -1/0/1."""
    return synth.write_geno_pair(str(tmp_path), np.ascontiguousarray(M.T.astype(np.int8)), stem=stem)


def _close(got, want, what):
    """1e-6 relative; a statistic that is a sum with cancellation (a_i = m_i . v) also gets fp64's own floor against the largest."""
    got, want = np.ravel(got), np.ravel(want)
    err = np.abs(got - want)
    bad = err > REL * np.abs(want) + 1e-12 * np.abs(want).max()
    print("%s: max relative difference %.3e" % (what, np.max(err / np.maximum(np.abs(want), 1e-12 * np.abs(want).max()))))
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:5])


def test_find_qtl_with_Z_matches_the_dense_model_on_both_scans(golden, tmp_path):
    M, ind, y, X, _ = rm_fixture(golden)
    Mk, indk, _ = drop_empty(M, ind)
    Mk = Mk.copy()
    Mk[:, 60] = 1.0                                                    # a monomorphic marker: in the column space of the intercept
    t, L = Mk.shape
    geno = _files(tmp_path, Mk)
    K = r_api.calcMMt(geno, 8.0, 1, np.array([NA]), True)
    np.testing.assert_allclose(K, kinship(Mk), rtol=1e-14)
    Z = dense_Z(indk, t)
    zm = host_model.ZModel(K, indk)
    rcpp_api.spectral_prepare(geno["asciifileMt"], (L, t), zm.spectral_basis()[0], 8.0)
    live = np.arange(L) != 60
    for Xc, varE, varG in ((X, 0.49, 1.3), (np.column_stack([X, Mk[indk, 47]]), 1.7, 0.2)):
        a, vara, _, _ = dense_scan(Mk, Z, K, Xc, y, varE, varG)
        use = live & (vara > 1e-9 * vara.max())                        # 47 once it is in the model
        want = tsq_argmax(np.where(use, a, 0.0), np.where(use, vara, 0.0)) + 1
        idx, st = r_api.find_qtl(geno, 8.0, np.array([NA]), K, None, varE, varG, Xc, 1, True, y, Zmat=zm, return_stats=True)
        _close(st["a"].ravel()[use], a[use], "a (reference-shaped scan)")
        _close(st["vara"].ravel()[use], vara[use], "vara (reference-shaped scan)")
        assert idx == want
        print("certificate (re-evaluated, flagged, block fell back):", rcpp_api.last_scan_certificate())
        assert abs(st["vara"].ravel()[60]) <= REL * vara[use].max()    # the monomorphic marker: zero up to the scan's tolerance
        op = zm.spectral_operands(Xc, y, varE, varG)
        sp = rcpp_api.spectral_scan_weights(op["d"], op["Gy"], op["GX"], op["C"], op["c1"], varG, L)
        _close(sp["a"].ravel()[use], a[use], "a (spectral_scan_weights)")
        _close(sp["vara"].ravel()[use], vara[use], "vara (spectral_scan_weights)")
        with np.errstate(all="ignore"):
            tsq = sp["a"].ravel() ** 2 / sp["vara"].ravel()
        assert np.isnan(tsq[60]) and sp["vara"].ravel()[60] == 0.0     # masked like a marker already in the model
        assert int(np.flatnonzero(tsq == np.nanmax(tsq))[0]) + 1 == want
        # the ind_of_obs vector instead of the kept ZModel is the same call
        assert r_api.find_qtl(geno, 8.0, np.array([NA]), K, None, varE, varG, Xc, 1, True, y, Zmat=indk) == idx
    masked = rcpp_api.spectral_scan_weights(op["d"], op["Gy"], op["GX"], op["C"], op["c1"], varG, L, selected_loci=np.array([3.0, 9.0]))
    assert masked["a"].ravel()[[3, 9]].tolist() == [0.0, 0.0] and masked["vara"].ravel()[[3, 9]].tolist() == [0.0, 0.0]
    rcpp_api.drop_cache()


def test_AM_with_identity_Z_is_AM(golden, tmp_path):
    g = golden("genoDemo_150x4998")
    geno = _files(tmp_path, g["M8"])
    y, X = g["y"].astype(np.float64), g["X"]
    ref = am.AM(y, X, geno, maxit=6)
    res = am.AM(y, X, geno, maxit=6, Zmat=np.eye(150))
    assert res["selected_loci"] == ref["selected_loci"] and res["all_picks"] == ref["all_picks"]
    np.testing.assert_allclose(res["extBIC"], ref["extBIC"], rtol=REL)
    assert res["indxNA"].size == 0 and res["indxNA_obs"].size == 0
    rcpp_api.drop_cache()


def test_AM_with_rows_of_identity_removed_is_AM_with_missing_records(golden, tmp_path):
    """Pins "an individual without a record leaves the genotypes" and the renumbering of ind_of_obs over the view."""
    g = golden("genoDemo_150x4998")
    geno = _files(tmp_path, g["M8"])
    y, X = g["y"].astype(np.float64), g["X"]
    gone = np.sort(np.random.default_rng(3).choice(150, 15, replace=False))
    y_na = y.copy()
    y_na[gone] = np.nan
    ref = am.AM(y_na, X, geno, maxit=6)
    keep = np.setdiff1d(np.arange(150), gone)
    for backend in (am.HipBackend(), am.SpectralBackend()):
        res = am.AM(y[keep], X[keep], geno, maxit=6, Zmat=np.eye(150)[keep], backend=backend)
        assert res["selected_loci"] == ref["selected_loci"] and res["all_picks"] == ref["all_picks"]
        assert res["indxNA"].tolist() == ref["indxNA"].tolist() == (gone + 1)[::-1].tolist()
        assert res["dim_of_ascii_M"] == ref["dim_of_ascii_M"] == [135, 4998]
        np.testing.assert_allclose(res["extBIC"], ref["extBIC"], rtol=REL)
    rcpp_api.drop_cache()


def test_AM_with_replicates_follows_the_dense_oracle_on_both_backends(golden, tmp_path):
    M, ind, y, X, planted = rm_fixture(golden)
    y = y.copy()
    y[5] = np.nan                                                      # one replicate of an individual that has others
    assert np.sum(ind == ind[5]) > 1
    geno = _files(tmp_path, M)
    keep = ~np.isnan(y)
    Mk, indk, _ = drop_empty(M, ind[keep])
    picks, trace = dense_AM(y[keep], X[keep], Mk, indk, maxit=6)
    out = []
    for backend, Zmat in ((am.HipBackend(), ind), (am.SpectralBackend(), dense_Z(ind, 150))):
        res = am.AM(y, X, geno, maxit=6, backend=backend, Zmat=Zmat)
        assert res["indxNA"].tolist() == [94, 8] and res["indxNA_obs"].tolist() == [6]   # the individual of record 6 stays
        assert res["all_picks"] == picks
        np.testing.assert_allclose(res["extBIC_trace"], trace, rtol=REL)
        out.append(res)
    assert out[0]["selected_loci"] == out[1]["selected_loci"]
    assert set(p + 1 for p in planted) <= set(out[0]["selected_loci"])
    rcpp_api.drop_cache()


def planted_case(n=400, L=20000, reps=5, nqtl=5, seed=21):
    """synth.py genotypes, `reps` records per individual, nqtl planted markers with effects large enough for the dense oracle to
    select every one of them (checked on the CPU when this was written; the effects were set by that, not the assertion)."""
    Mt8 = synth.genotypes_marker_major(n, L, seed=seed)
    M = Mt8.T.astype(np.float64)
    rng = np.random.default_rng(seed)
    planted = np.linspace(0, L - 1, nqtl + 2, dtype=np.int64)[1:-1]
    beta = 1.2 * np.where(np.arange(nqtl) % 2 == 0, 1.0, -1.0)
    ind = np.repeat(np.arange(n), reps)
    gen = M[:, planted] @ beta + 0.5 * rng.standard_normal(n)
    y = 1.0 + gen[ind] + 0.8 * rng.standard_normal(ind.size)
    return Mt8, M, ind, y, np.ones((ind.size, 1)), [int(p) for p in planted]


def test_planted_qtl_recovered_with_five_records_per_individual(tmp_path):
    Mt8, M, ind, y, X, planted = planted_case()
    picks, _ = dense_AM(y, X, M, ind, maxit=8)
    assert set(p + 1 for p in planted) <= set(picks)                   # the oracle alone finds them
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    for backend in (am.HipBackend(), am.SpectralBackend()):
        res = am.AM(y, X, geno, maxit=8, backend=backend, Zmat=ind)
        assert res["all_picks"] == picks
        assert set(p + 1 for p in planted) <= set(res["selected_loci"])
    rcpp_api.drop_cache()


def test_spectral_scan_and_spectral_scan_weights_are_one_path(golden, tmp_path):
    """eagle_spectral_scan prepares d, G, C, c1 (eagle_spectral_host_operands, an internal symbol of the library) and runs the
    pass / finish sequence eagle_spectral_scan_weights runs: fed the same operands the two return the same bits."""
    g = golden("genoDemo_150x4998")
    n, L = g["M8"].shape
    geno = _files(tmp_path, g["M8"])
    K = r_api.calcMMt(geno, 8.0, 1, np.array([NA]), True)
    lam, U = np.linalg.eigh(K)
    rcpp_api.spectral_prepare(geno["asciifileMt"], (L, n), U, 8.0)
    X = np.column_stack([g["X"], g["M8"][:, [17, 900]].astype(np.float64)])
    UtX, Uty = np.asfortranarray(U.T @ X), U.T @ g["y"].astype(np.float64).ravel()
    p, varE, varG = X.shape[1], 0.7, 1.9
    lib = _lib.load()
    c_dp = C.POINTER(C.c_double)
    fn = lib.eagle_spectral_host_operands
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_long, c_dp, c_dp, c_dp, C.c_long, C.c_double, C.c_double, C.c_int, c_dp, c_dp, c_dp, c_dp]
    NC, n_pad = 16, 256
    d, G, Cm, c1 = np.zeros(n_pad), np.zeros((n_pad, NC)), np.zeros((p, p)), np.zeros(p)
    ptr = lambda a: a.ctypes.data_as(c_dp)
    assert fn(None, n, ptr(np.ascontiguousarray(lam)), ptr(UtX), ptr(Uty), p, varE, varG, NC, ptr(d), ptr(G), ptr(Cm), ptr(c1)) == 0
    sel = np.array([5.0, 2000.0])
    for s in (NA, sel):
        ref = rcpp_api.spectral_scan(lam, UtX, Uty, varE, varG, L, selected_loci=s)
        res = rcpp_api.spectral_scan_weights(d[:n], G[:n, 0], G[:n, 1:1 + p], Cm, c1, varG, L, selected_loci=s)
        assert np.array_equal(ref["a"], res["a"]) and np.array_equal(ref["vara"], res["vara"])
    assert np.all(ref["a"].ravel()[[5, 2000]] == 0.0) and np.count_nonzero(ref["a"]) > L // 2
    with pytest.raises(_lib.EagleError):
        rcpp_api.spectral_scan_weights(d[:n], G[:n, 0], np.zeros((n, 32)), np.eye(32), np.zeros(32), varG, L)
    rcpp_api.drop_cache()
