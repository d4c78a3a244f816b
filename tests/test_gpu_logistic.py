"""Logistic regression per marker on the GPU: eagle_logistic (k_logit_irls<0|1|2>, csrc/eagle_logit.hip) and the r_api interface on top.

Expected values: the 40-digit roots of tests/logistic_truth.py (stored in tests/golden/logistic_truth.npz, keyed by a digest of each
panel's inputs; tests/test_logistic_host.py recomputes entries live), the closed forms of saturated 2 x 2 tables, CaseControl's trend
test for the score, and r_api.logistic_host for the codes.  The bounds are logistic_truth.ml_bounds / firth_bounds: the stop rule
plus the fixed point's sensitivity to the rounding of U, worked out per marker from the truth.  Device against device (routes, marker
order) is ==.  Every call uses tol = 1e-10."""
import math
import os

import numpy as np
import pytest

import logistic_truth as truth
from test_gpu_marker_qc import ingest_text

TOL = 1e-10


def mono_rows(Mt8, st):
    return np.array([np.ptp(Mt8[m, st >= 0]) == 0 for m in range(Mt8.shape[0])])


def check_panel(tmp_path, name):
    from eagleeverything_amd import r_api, rcpp_api, synth
    Mt8, st, X, firth_rows, t = truth.golden(name)
    L, n = Mt8.shape
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    fMt, dims = geno["asciifileMt"], (n, L)
    stat0, info0 = rcpp_api.logistic(fMt, dims, st, X, firth=0, tol=TOL)
    stat2, info2 = rcpp_api.logistic(fMt, dims, st, X, firth=2, tol=TOL)
    assert stat0.shape == (L, 4) and info0.shape == (L, 2) and stat0.dtype == np.float64 and info0.dtype == np.int32
    hstat, hinfo = r_api.logistic_host(Mt8, st, X, 0, TOL, 50)

    # ---- maximum likelihood against the truth, wherever its fit exists with a clear margin and cond(I) <= 1e6
    good = (t["ok"] == 1) & (t["maxeta"] <= truth.ETA_CLEAR) & (t["cond"] <= 1e6)
    if L >= 8:
        assert good.mean() > 0.95, (name, good.mean())
    else:
        assert good.all()
    bg, rse, rll = truth.ml_bounds(n, TOL, {k: v[good] for k, v in t.items()})
    for stat, info in ((stat0, info0), (stat2, info2)):                       # the fallback leaves a converged ML fit alone
        assert np.all(info[good, 0] == 0), (name, info[good, 0].max())
        eg = np.abs(stat[good, 0] - t["gamma"][good])
        es = np.abs(stat[good, 1] / t["se"][good] - 1.0)
        el = np.abs(stat[good, 3] / t["ll"][good] - 1.0)
        print("%s: worst gamma error / bound %.3g, se %.3g, loglik %.3g" % (name, (eg / bg).max(), (es / rse).max(), (el / rll).max()))
        assert np.all(eg <= bg) and np.all(es <= rse) and np.all(el <= rll), name
        assert np.all(info[good, 1] >= 2) and np.all(info[good, 1] <= 50)
    # the score against the restatement's: two fp64 evaluations of the same sums (logistic_truth.score_bounds)
    fin = np.isfinite(hstat[:, 2])
    assert np.array_equal(fin, np.isfinite(stat0[:, 2])) and np.array_equal(fin, ~mono_rows(Mt8, st))
    sb = truth.score_bounds(Mt8, st, X, r_api.logistic_null_host(X[st >= 0], st[st >= 0]), hstat[:, 2])
    assert np.all(np.abs(stat0[fin, 2] - hstat[fin, 2]) <= sb[fin]), name
    assert np.array_equal(stat2[:, 2], stat0[:, 2], equal_nan=True)           # the fallback keeps the first evaluation's score

    # ---- codes
    mono = mono_rows(Mt8, st)
    assert np.all(info0[mono, 0] == 2) and np.all(info2[mono, 0] == 2) and np.all(info0[mono, 1] == 1)
    assert np.all(np.isnan(stat0[mono])) and np.all(np.isnan(stat2[mono]))
    clear = good | mono
    assert np.array_equal(info0[clear, 0], hinfo[clear, 0]), name
    bad0 = info0[:, 0] != 0
    assert np.all(np.isnan(stat0[bad0][:, [0, 1, 3]]))
    assert np.array_equal(info2[:, 0] >= 256, bad0 & ~mono)                    # restarted exactly where ML failed after its first evaluation
    if L >= 8:
        # the planted separated marker: ML says so, the fallback restarts it (with covariates Firth's iteration is slow on a separated
        # marker and may use up max_iter: code 257; the intercept-only panel c1 and the saturated tables below hold it to its closed form)
        assert mono[L - 3:].all() and info0[L - 4, 0] in (1, 3) and info2[L - 4, 0] in (256, 257)
        assert np.isfinite(stat2[L - 4, 0]) == (info2[L - 4, 0] == 256)

    # ---- Firth against the truth
    if firth_rows:
        stat1, info1 = rcpp_api.logistic(fMt, dims, st, X, firth=1, tol=TOL, max_iter=200)
        assert np.all(info1[:, 0] >= 256) and np.all(info1[mono, 0] == 258)
        rows = [m for m in firth_rows if t["f_ok"][m] == 1 and t["f_cond"][m] <= 1e6]
        assert len(rows) >= len(firth_rows) - 1
        for m in rows:
            assert t["f_ratio"][m] <= 0.9, (name, m, t["f_ratio"][m])
            fg, fse = truth.firth_bounds(n, TOL, t, m)
            assert info1[m, 0] == 256, (name, m, info1[m])
            assert abs(stat1[m, 0] - t["f_gamma"][m]) <= fg, (name, m, stat1[m, 0] - t["f_gamma"][m], fg)
            assert abs(stat1[m, 1] - t["f_se"][m]) <= fse * t["f_se"][m], (name, m)
            if info2[m, 0] == 256:                                             # the fallback's fit is this fit
                assert abs(stat2[m, 0] - t["f_gamma"][m]) <= fg and abs(stat2[m, 1] - t["f_se"][m]) <= fse * t["f_se"][m]
    rcpp_api.drop_cache()
    return geno, st, X, stat0, info0


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.gpu
@pytest.mark.parametrize("n", truth.NS)
def test_gpu_logistic_every_n(tmp_path, n):
    """The 4-individual MFMA step, the 64-individual chunk and ragged tails of 1 to 3, at L = 300 (75 workgroups)."""
    check_panel(tmp_path, "n%d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("L", truth.LS)
def test_gpu_logistic_every_L(tmp_path, L):
    """The four-marker workgroup edge, at n = 203."""
    check_panel(tmp_path, "L%d" % L)


@pytest.mark.gpu
@pytest.mark.parametrize("c", truth.CS)
def test_gpu_logistic_every_c(tmp_path, c):
    """No padding at p = 16, eleven zero columns at p = 5, fourteen at p = 2; at c = 1 the score is CaseControl's trend test."""
    from eagleeverything_amd import r_api
    geno, st, X, stat0, info0 = check_panel(tmp_path, "c%d" % c)
    if c == 1:
        trend = r_api.CaseControl(geno, np.where(st < 0, np.nan, st.astype(np.float64)))["trend"]
        ok = np.isfinite(trend)
        assert ok.sum() >= len(trend) - 3
        assert np.all(np.abs(stat0[ok, 2] - trend[ok]) <= 1e-11 * trend[ok])
        # the planted separated marker, g = 1 on the cases and 0 on the controls: the table (R, 0; 0, S) with a half added to every cell
        from eagleeverything_amd import rcpp_api
        L = len(trend)
        stat2, info2 = rcpp_api.logistic(geno["asciifileMt"], (len(st), L), st, X, firth=2, tol=TOL)
        R, S = int((st == 1).sum()), int((st == 0).sum())
        assert info0[L - 4, 0] in (1, 3) and info2[L - 4, 0] == 256
        assert abs(stat2[L - 4, 0] - math.log((R + .5) * (S + .5) / (.5 * .5))) <= 1e-8


# ------------------------------------------------------------------------------------------------ 2. closed forms
@pytest.mark.gpu
def test_gpu_logistic_saturated_tables(tmp_path):
    """Intercept plus a 0 / 2-only marker: ML = log(ad / bc) / 2 with Woolf's se halved, Firth = the same with a half added to every
    cell; a zero cell separates (code 3 or 1) and the fallback returns the half-added estimate under code 256."""
    from eagleeverything_amd import rcpp_api, synth
    R, S, spare = 12, 13, 5
    st = np.array([1] * R + [0] * S + [-1] * spare, dtype=np.int32)
    tables = [(7, 4), (7, 0), (12, 8), (12, 0), (3, 11)]                      # (carriers among the cases, among the controls)
    n = st.size
    Mt8 = np.full((len(tables), n), -1, dtype=np.int8)
    for m, (a, b) in enumerate(tables):
        Mt8[m, :a] = 1
        Mt8[m, R:R + b] = 1
        Mt8[m, R + S:] = [1, 0, -1, 0, 1]                                     # the unused individuals are not in the table
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    X = np.ones((n, 1))
    out = {f: rcpp_api.logistic(geno["asciifileMt"], (n, len(tables)), st, X, firth=f, tol=TOL, max_iter=100) for f in (0, 1, 2)}
    for m, (a, b) in enumerate(tables):
        c, d = R - a, S - b
        half = 0.5 * math.log((a + .5) * (d + .5) / ((b + .5) * (c + .5)))
        if min(a, b, c, d) > 0:
            for f in (0, 2):
                stat, info = out[f]
                assert info[m, 0] == 0
                assert abs(stat[m, 0] - 0.5 * math.log(a * d / (b * c))) <= 1e-9
                assert abs(stat[m, 1] - 0.5 * math.sqrt(1 / a + 1 / b + 1 / c + 1 / d)) <= 1e-9
        else:
            # no carrier among the controls: gamma runs away, code 3 (or 1); no case outside the carriers: the intercept runs away and
            # gamma's column becomes the intercept's to the resolution of fp64 first, code 2 after the first evaluation
            assert out[0][1][m, 0] in ((1, 3) if b == 0 else (1, 2, 3)) and out[0][1][m, 1] > 1
            assert np.isnan(out[0][0][m, 0]) and np.isfinite(out[0][0][m, 2])
            assert out[2][1][m, 0] == 256 and abs(out[2][0][m, 0] - half) <= 1e-8
        assert out[1][1][m, 0] == 256 and abs(out[1][0][m, 0] - half) <= 1e-8
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 3. routes
@pytest.mark.gpu
def test_gpu_logistic_routes_and_marker_order(golden, tmp_path, monkeypatch):
    """Resident, streamed in row windows, text without a sidecar and the same panel with its markers reversed: the same bits, because a
    wave's result depends on its marker's row alone."""
    from eagleeverything_amd import rcpp_api
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    X = truth.covariates(n, 4, 41)
    st = truth.draw_status(X, 42)
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    rev = ingest_text(tmp_path, "r", np.ascontiguousarray(M8[:, ::-1]))
    fMt = geno["asciifileMt"]
    stat, info = rcpp_api.logistic(fMt, (n, L), st, X, tol=TOL)               # the image the converter left resident
    assert (info[:, 0] == 0).mean() > 0.9
    rstat, rinfo = rcpp_api.logistic(rev["asciifileMt"], (n, L), st, X, tol=TOL)
    assert np.array_equal(rstat[::-1], stat, equal_nan=True) and np.array_equal(rinfo[::-1], info)
    rcpp_api.drop_cache()                                                     # from the sidecar, made resident
    s2, i2 = rcpp_api.logistic(fMt, (n, L), st, X, tol=TOL)
    assert np.array_equal(s2, stat, equal_nan=True) and np.array_equal(i2, info)
    rcpp_api.drop_cache()                                                     # in row windows of 256 markers
    n_pad = (n + 255) // 256 * 256
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr((256 * n_pad - 16) / 1e9))
    s3, i3 = rcpp_api.logistic(fMt, (n, L), st, X, tol=TOL)
    assert np.array_equal(s3, stat, equal_nan=True) and np.array_equal(i3, info)
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")                              # the same windows from the text
    s4, i4 = rcpp_api.logistic(fMt, (n, L), st, X, tol=TOL)
    assert np.array_equal(s4, stat, equal_nan=True) and np.array_equal(i4, info)
    rcpp_api.drop_cache()


@pytest.mark.gpu
def test_gpu_logistic_on_view_alias(golden, tmp_path, monkeypatch):
    from eagleeverything_amd import am, rcpp_api
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    na = np.array([1, 2, 57, 130, 203])                                       # 1-based, as R hands them over
    kept = np.setdiff1d(np.arange(n), na - 1)
    sub = ingest_text(tmp_path, "k", np.ascontiguousarray(M8[kept]))           # the kept individuals as a panel of their own
    X = truth.covariates(n - 5, 3, 51)                                        # one row per KEPT individual
    st = truth.draw_status(X, 52)
    want = rcpp_api.logistic(sub["asciifileMt"], (n - 5, L), st, X, tol=TOL)
    view = am.reshape_geno(geno, na, view=True)
    assert list(view["dim_of_ascii_M"]) == [n - 5, L]
    got = rcpp_api.logistic(view["asciifileMt"], (n - 5, L), st, X, tol=TOL)
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])
    rcpp_api.drop_cache()                                                     # the same alias from the source's sidecar, in windows
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr(2 * 256 * 256 / 1e9))
    got = rcpp_api.logistic(view["asciifileMt"], (n - 5, L), st, X, tol=TOL)
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError):
        rcpp_api.logistic(view["asciifileMt"], (n - 5, L), np.zeros(n), np.ones((n, 1)), tol=TOL)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 4. the interface
@pytest.mark.gpu
def test_gpu_Logistic_end_to_end(tmp_path):
    from scipy import special
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    n, L, causal = 257, 200, 77
    Mt8 = synth.genotypes_marker_major(n, L, seed=61)
    Mt8[causal] = synth.genotypes_marker_major(n, 1, seed=62, first_marker=5000)[0]
    pcs = np.random.default_rng(63).standard_normal((n, 2))
    X = am.add_pcs(np.ones(n), {"pcs": pcs})
    assert X.shape == (n, 3)
    st = truth.draw_status(X, 64, extra=1.6 * (Mt8[causal] + 1.0) - 1.6).astype(np.float64)
    st[st < 0] = np.nan
    Mt8[5] = np.where(st == 1, 1, -1)                                        # separated: the carriers are the cases
    assert all(np.ptp(Mt8[m, np.isfinite(st)]) > 0 for m in range(L))
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    Xn = X.copy()
    dropped = [i for i in range(n) if np.isfinite(st[i])][3]
    Xn[dropped, 2] = np.nan
    out = r_api.Logistic(geno, st, Xn, tol=TOL, max_iter=200)       # Firth needs about 100 evaluations on the separated marker
    sv = np.where(np.isnan(st), -1, st).astype(np.int32)
    sv[dropped] = -1
    assert out["n_used"] == int((sv >= 0).sum()) == int(np.isfinite(st).sum()) - 1
    p = out["p"].copy()
    p[5] = np.nan                                                            # the planted separated marker aside
    assert int(np.nanargmin(p)) == causal and p[causal] < 1e-4 and out["beta"][causal] > 0
    X0 = np.where(np.isnan(Xn), 0.0, Xn)
    assert np.allclose(out["beta0"], r_api.logistic_null_host(X0[sv >= 0], sv[sv >= 0]), rtol=0, atol=1e-12)
    ml_stat, ml_info = rcpp_api.logistic(geno["asciifileMt"], (n, L), sv, X0, firth=0, tol=TOL, max_iter=200)
    assert np.array_equal(out["firth"], ml_info[:, 0] != 0) and out["firth"][5] and out["firth"].sum() < L // 10
    assert np.array_equal(out["code"] >= 256, out["firth"]) and out["iterations"].min() >= 2
    conv = out["code"] % 256 == 0
    assert conv[5] and np.isfinite(out["beta"][5]) and np.all(np.isnan(out["lrt"][out["firth"]]))
    ml = conv & ~out["firth"]
    assert np.array_equal(out["beta"][ml], ml_stat[ml, 0]) and np.array_equal(out["se"][ml], ml_stat[ml, 1])
    assert np.allclose(out["or"][conv], np.exp(out["beta"][conv])) and np.allclose(out["z"][conv], out["beta"][conv] / out["se"][conv])
    assert np.allclose(out["p"][conv], 2 * special.ndtr(-np.abs(out["z"][conv])))
    assert np.allclose(out["p_score"], special.chdtrc(1.0, out["score"]))
    assert np.all(out["lrt"][ml] > -1e-9) and np.allclose(out["p_lrt"][ml], special.chdtrc(1.0, np.maximum(out["lrt"][ml], 0)))
    # Wald, score and likelihood-ratio tests agree to first order on an ordinary marker
    m = int(np.flatnonzero(ml)[0])
    assert abs(out["z"][m] ** 2 - out["score"][m]) <= 0.5 * max(out["score"][m], 1.0)
    # intercept only, every marker by Firth, and the ML-only form
    o1 = r_api.Logistic(geno, st, firth="firth", tol=TOL)
    assert o1["firth"].all() and o1["beta0"].shape == (1,) and o1["n_used"] == int(np.isfinite(st).sum())
    o0 = r_api.Logistic(geno, st, firth="ml", tol=TOL)
    assert not o0["firth"].any() and o0["code"][5] in (1, 3) and np.isnan(o0["beta"][5])
    trend = r_api.CaseControl(geno, st)["trend"]
    assert np.all(np.abs(o0["score"] - trend) <= 1e-11 * trend)
    rcpp_api.drop_cache()
