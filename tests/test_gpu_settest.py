"""The set test on an MI355X (eagle_spectral_settest, k_settest_gram; include/eagle_hip.h section 1d''): every panel of
tests/settest_truth.py against the 40-digit truth with the bounds derived there, the scores and the diagonal of Phi against
eagle_spectral_scan, Phi symmetric with ==, equal bytes for a reversed list / a second call / a repeated set / single sets, the planted
degenerate markers, the argument errors that need a prepared context (the non-finite operands through the bound symbol, which the
Python wrapper would refuse first), and am.SetTest end to end.

The panels prepare Z on the fp64 MFMA (set_scan_mode(0)), as tests/test_gpu_lmm.py does: the truth's bounds carry fp64 rounding of the
operands, n 2^-53, and the default digit-slice build of Z is documented to n 2^-47.  SetTest end to end runs on the default build."""
import numpy as np
import pytest

import settest_truth as T
from eagleeverything_amd import am, r_api, rcpp_api, synth
from eagleeverything_amd._lib import EagleError
from test_settest_host import assert_meets_truth, operands

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


def _bytes(res, order=None):
    """The four outputs as bytes per set, in the order of `order` (positions in res)."""
    k = len(res["score"])
    order = range(k) if order is None else order
    return [(res["stat"][o].tobytes(), res["info"][o].tobytes(), res["score"][o].tobytes(), res["cov"][o].tobytes()) for o in order]


@pytest.mark.parametrize("name", T.all_panels())
def test_device_meets_truth(tmp_path, name):
    lam, U, UtX, Uty, Z, Mt8, X, y, st, om = operands(name)
    M, n = Mt8.shape
    _prepare(tmp_path, Mt8, U)
    res = rcpp_api.spectral_settest(lam, UtX, Uty, T.VAR_E, T.VAR_G, st, om, scores=True, cov=True)
    assert res["stat"].shape == (len(st), 7) and res["info"].shape == (len(st), 2)
    assert_meets_truth(name, res, print)
    for Phi in res["cov"]:
        assert (Phi == Phi.T).all()
    # the scores and the diagonal of Phi against the scan of the same operands: each within its bound of the truth
    scan = rcpp_api.spectral_scan(lam, UtX, Uty, T.VAR_E, T.VAR_G, M)
    t = T.golden(name)[0]                                                  # set 0: every marker, in order
    live = t["deg"] < 0.5
    a, vara = scan["a"].ravel(), scan["vara"].ravel()
    assert (np.abs(a - t["s"])[live] <= t["b_s"][live]).all() and (np.abs(vara - np.diag(t["Phi"]))[live] <= np.diag(t["b_Phi"])[live]).all()
    assert (np.abs(res["score"][0] - a)[live] <= 2 * t["b_s"][live]).all()
    assert (np.abs(np.diag(res["cov"][0]) - vara)[live] <= 2 * np.diag(t["b_Phi"])[live]).all()
    # equal bytes: the reversed list, a second call, a list with one set repeated, single sets, and without the optional outputs
    ref = _bytes(res)
    k = len(st)
    rev = rcpp_api.spectral_settest(lam, UtX, Uty, T.VAR_E, T.VAR_G, st[::-1], om[::-1], scores=True, cov=True)
    assert _bytes(rev, range(k - 1, -1, -1)) == ref
    assert _bytes(rcpp_api.spectral_settest(lam, UtX, Uty, T.VAR_E, T.VAR_G, st, om, scores=True, cov=True)) == ref
    rep = rcpp_api.spectral_settest(lam, UtX, Uty, T.VAR_E, T.VAR_G, [st[0], st[1], st[0], st[2], st[0]], [om[0], om[1], om[0], om[2], om[0]],
                                    scores=True, cov=True)
    assert _bytes(rep) == [ref[0], ref[1], ref[0], ref[2], ref[0]]
    for o in range(k):
        assert _bytes(rcpp_api.spectral_settest(lam, UtX, Uty, T.VAR_E, T.VAR_G, [st[o]], [om[o]], scores=True, cov=True)) == [ref[o]]
    bare = rcpp_api.spectral_settest(lam, UtX, Uty, T.VAR_E, T.VAR_G, st, om)
    assert sorted(bare) == ["info", "stat"] and bare["stat"].tobytes() == res["stat"].tobytes() and np.array_equal(bare["info"], res["info"])
    rcpp_api.drop_cache()


def test_planted_degenerate_markers(tmp_path):
    lam, U, UtX, Uty, Z, Mt8, X, y, st, om = operands("deg")
    _prepare(tmp_path, Mt8, U)
    res = rcpp_api.spectral_settest(lam, UtX, Uty, T.VAR_E, T.VAR_G, st, om, scores=True, cov=True)
    M = Mt8.shape[0]
    assert list(res["info"][:, 0]) == [0, 2, 0] and list(res["info"][:, 1]) == [M - 2, 0, 1]
    for o in (0, 1):                                                       # the monomorphic marker and the one equal to a column of X
        assert (res["score"][o][:2] == 0.0).all() and (res["cov"][o][:2, :] == 0.0).all() and (res["cov"][o][:, :2] == 0.0).all()
    assert np.isnan(res["stat"][1]).all() and np.isfinite(res["stat"][[0, 2]]).all()
    assert (np.diag(res["cov"][0])[2:] > 0).all() and (res["score"][0][2:] != 0.0).all()
    host = r_api.settest_host(lam, UtX, Uty, Z, T.VAR_E, T.VAR_G, st, om)
    np.testing.assert_array_equal(res["info"], host["info"])
    rcpp_api.drop_cache()


def test_argument_errors_that_need_a_prepared_context(tmp_path):
    lam, U, UtX, Uty, Z, Mt8, X, y, st, om = operands("m17")
    M, n = Mt8.shape
    rcpp_api.close_all()                                                   # a context without a prepare
    for d in ("s", "t"):
        (tmp_path / d).mkdir()
    with pytest.raises(EagleError) as e:
        rcpp_api.spectral_settest(lam, UtX, Uty, 1.0, 1.0, st, om)
    assert e.value.code == -3 and "eagle_spectral_prepare has not run" in e.value.text
    _prepare(tmp_path, Mt8, U)
    empty = rcpp_api.spectral_settest(lam, UtX, Uty, 1.0, 1.0, [], scores=True, cov=True)
    assert empty["stat"].shape == (0, 7) and empty["info"].shape == (0, 2) and empty["score"] == [] and empty["cov"] == []
    bad_lam = lam.copy()
    bad_lam[5] = -4.0
    collinear = np.column_stack([UtX, UtX[:, 0] * 2.0])
    for kw, text in ((dict(sets=[[0, M]]), "marker index out of range"), (dict(lam=bad_lam), "varE + varG * lambda_k must be positive"),
                     (dict(varE=-5.0), "varE + varG * lambda_k must be positive"), (dict(UtX=collinear), "X^T H^-1 X is not positive definite"),
                     (dict(lam=lam[:15], UtX=np.ones((15, 14)), Uty=Uty[:15]), "n <= c + 1")):
        args = dict(lam=lam, UtX=UtX, Uty=Uty, varE=1.0, varG=1.0, sets=[[0, 1]])
        args.update(kw)
        if "n <= c + 1" == text:                                           # the resident Z decides n: prepare a panel of 15 individuals
            rcpp_api.spectral_prepare(synth.write_geno_pair(str(tmp_path / "s"), Mt8[:, :15].copy())["asciifileMt"], (M, 15), np.eye(15), 8.0)
        with pytest.raises(EagleError) as e:
            rcpp_api.spectral_settest(**args)
        assert e.value.code == -3 and text in e.value.text, (text, e.value.text)
    rcpp_api.spectral_prepare(synth.write_geno_pair(str(tmp_path / "t"), Mt8)["asciifileMt"], (M, n), U, 8.0, device=(0, 0))
    with pytest.raises(EagleError) as e:
        rcpp_api.spectral_settest(lam, UtX, Uty, 1.0, 1.0, [[0, 1]], device=(0, 0))
    assert e.value.code == -3 and "multi-device" in e.value.text
    rcpp_api.close_all()


def test_non_finite_operands_reach_the_library(tmp_path):
    """rcpp_api.spectral_settest refuses non-finite input before the library is called, so the library's own checks -- which need the n
    of the resident Z and cannot be made with ctx == NULL -- are reached through the bound symbol on a prepared context: a NaN or an
    infinity in lambda, in UtX and in Uty are EAGLE_ERR_ARG with their text, and nothing is written."""
    import ctypes as C
    from eagleeverything_amd import _lib
    from eagleeverything_amd._lib import c_dp, c_lp
    lam, U, UtX, Uty, Z, Mt8, X, y, st, om = operands("m17")
    _prepare(tmp_path, Mt8, U)
    lib, ctx = _lib.load(), rcpp_api.context(0)
    ptr, idx, w = rcpp_api.settest_csr([[0, 1, 2]])
    c = UtX.shape[1]
    good = dict(lam=np.ascontiguousarray(lam, dtype=np.float64), UtX=np.asfortranarray(UtX, dtype=np.float64), Uty=np.ascontiguousarray(Uty, dtype=np.float64))

    def call(**kw):
        a = {k: v.copy(order="K") for k, v in good.items()}
        for k, (pos, v) in kw.items():
            a[k].reshape(-1, order="F")[pos] = v
        stat, info = np.full(7, -1.0), np.full(2, -1, dtype=np.int32)
        rc = lib.eagle_spectral_settest(ctx, a["lam"].ctypes.data_as(c_dp), a["UtX"].ctypes.data_as(c_dp), a["Uty"].ctypes.data_as(c_dp), c, 1.0, 1.0, 1,
                                        ptr.ctypes.data_as(c_lp), idx.ctypes.data_as(c_lp), w.ctypes.data_as(c_dp), stat.ctypes.data_as(c_dp),
                                        info.ctypes.data_as(C.POINTER(C.c_int32)), None, None)
        return rc, lib.eagle_last_error(ctx).decode(), stat, info

    rc, _, stat, info = call()
    assert rc == 0 and info[0] == 0 and np.isfinite(stat).all()
    n = lam.size
    for kw, text in ((dict(lam=(3, np.nan)), "varE + varG * lambda_k must be positive and finite"),
                     (dict(lam=(n - 1, np.inf)), "varE + varG * lambda_k must be positive and finite"),
                     (dict(lam=(0, -np.inf)), "varE + varG * lambda_k must be positive and finite"),
                     (dict(UtX=(5, np.nan)), "a non-finite entry of UtX or Uty"), (dict(UtX=(c * n - 1, -np.inf)), "a non-finite entry of UtX or Uty"),
                     (dict(Uty=(0, np.inf)), "a non-finite entry of UtX or Uty"), (dict(Uty=(n - 1, np.nan)), "a non-finite entry of UtX or Uty")):
        rc, msg, stat, info = call(**kw)
        assert rc == -3 and msg == "spectral_settest: " + text, (kw, rc, msg)
        assert (stat == -1.0).all() and (info == -1).all()
    rcpp_api.drop_cache()


def test_settest_end_to_end(tmp_path, monkeypatch):
    """40 windows of 16 markers, n = 300, on the default Z build; window 17 carries three planted effects of mixed sign: it has the
    smallest p_skat, it is refined, and p_skat_liu is skat_pvalue of the host restatement's traces within the propagated bound.

    The bound.  The device's Z is the digit-slice build, |Z - Mt U| <= zeta = n 2^-47 entrywise (include/eagle_hip.h section 1d), so a
    row differs by at most sqrt(n) zeta in norm.  With Pt = D - D Xt (Xt' D Xt)^-1 Xt' D, 0 <= Pt <= max d, s_j = varG z_j' Pt yt and
    Phi_ij = varG^2 z_i' Pt z_j move, to first order, by at most
        ds = varG max d sqrt(n) zeta |yt|,      dPhi_ij = varG^2 max d sqrt(n) zeta (|z_i| + |z_j|),
    and with weights 1: dQ = 2 sum |s_j| ds, dc_1 = sum dPhi_ii, dc_r = r |Phi|_F^(r-1) |dPhi|_F (settest_truth's trace bound).  The two
    fp64 evaluations themselves are held by settest_truth to 8 (n + 16) 2^-53 = 2^-41.7 relative on the absolute Gram, an eighth of
    zeta = 2^-38.8 on entries of z of order 1; they and the second-order terms are covered by asserting TWICE the first-order bound.
    Liu's p then moves by at most sum_v |dp/dv| dv, the derivatives by central differences."""
    n, L, W = 300, 640, 16
    Mt8 = synth.genotypes_marker_major(n, L, seed=11)
    rng = np.random.default_rng(12)
    X = np.column_stack([np.ones(n), rng.standard_normal(n)])
    first = 17 * W
    y = X @ [1.0, 0.3] + 0.05 * (Mt8.astype(np.float64).T @ rng.standard_normal(L)) + 1.0 * rng.standard_normal(n)
    # K is made of these 640 markers alone and absorbs much of a single marker's effect at n = 300: the planted effects are large
    y = y + 1.5 * Mt8[first + 2] - 1.6 * Mt8[first + 7] + 1.4 * Mt8[first + 11]
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    prepares = []
    real = rcpp_api.spectral_prepare
    monkeypatch.setattr(rcpp_api, "spectral_prepare", lambda *a, **k: (prepares.append(1), real(*a, **k))[1])
    be = am.SpectralBackend()
    g = am.GWAS(y, X, geno, exact="none", backend=be)
    win = r_api.sets_from_windows(L, size=W)
    out = r_api.SetTest(y, X, geno, win, backend=be)
    assert len(prepares) == 1 and len(win["sets"]) == 40                   # the resident Z of GWAS() is reused
    print("p_skat", out["p_skat"][17], "p_skat_liu", out["p_skat_liu"][17], "p_burden", out["p_burden"][17], "second", np.sort(out["p_skat"])[1])
    assert int(np.nanargmin(out["p_skat"])) == 17 and out["refined"][17] and out["p_skat"][17] < 1e-3 and (out["code"] == 0).all()
    assert (out["n_used"] == W).all() and (out["n_markers"] == W).all() and out["null"] == g["null_reml"]
    assert np.array_equal(out["refined"], out["p_skat_liu"] < 1e-3) and (out["p_skat"][~out["refined"]] == out["p_skat_liu"][~out["refined"]]).all()
    assert out["p_burden"][17] > out["p_skat"][17]                         # effects of mixed sign: the burden test loses them
    lam, U = be.eig
    UtX, Uty, Zh = U.T @ X, U.T @ y, Mt8.astype(np.float64) @ U
    ve, vg = out["null"]["ve"], out["null"]["vg"]
    host = r_api.settest_host(lam, UtX, Uty, Zh, ve, vg, win["sets"])
    np.testing.assert_array_equal(out["Q"], rcpp_api.spectral_settest(lam, UtX, Uty, ve, vg, win["sets"])["stat"][:, 0])
    zeta, dmax, worst = n * 2.0 ** -47, float(np.max(1.0 / (ve + vg * lam))), 0.0
    for o, js in enumerate(win["sets"]):
        want = np.concatenate([[host["stat"][o, 0]], host["stat"][o, 3:7]])           # Q, c_1 .. c_4
        zn = np.linalg.norm(Zh[js], axis=1)
        ds = vg * dmax * np.sqrt(n) * zeta * float(np.linalg.norm(Uty))
        dPhi = vg * vg * dmax * np.sqrt(n) * zeta * (zn[:, None] + zn[None, :])
        nA, nd = float(np.linalg.norm(host["cov"][o])), float(np.linalg.norm(dPhi))
        dv = 2.0 * np.array([2.0 * np.sum(np.abs(host["score"][o])) * ds, np.trace(dPhi), 2 * nA * nd, 3 * nA ** 2 * nd, 4 * nA ** 3 * nd])
        p0, bound = r_api.skat_pvalue(want[0], c=want[1:]), 0.0
        for j in range(5):
            h = 1e-6 * abs(want[j])
            up, dn = want.copy(), want.copy()
            up[j] += h
            dn[j] -= h
            bound += abs(r_api.skat_pvalue(up[0], c=up[1:]) - r_api.skat_pvalue(dn[0], c=dn[1:])) / (2 * h) * dv[j]
        assert abs(out["p_skat_liu"][o] - p0) <= bound, (o, out["p_skat_liu"][o], p0, bound)
        worst = max(worst, abs(out["p_skat_liu"][o] - p0) / bound)
    print("largest |p_skat_liu - host| / bound %.3g" % worst)
    rcpp_api.drop_cache()
