"""CPU: r_api.settest_host, the numpy restatement of include/eagle_hip.h section 1d'', against the 40-digit truth of
tests/settest_truth.py with the bounds derived there (no tuned number); golden entries recomputed live; a set of one marker against the
score test of the scan; the p-value functions (the modified Liu form against chi^2 for equal eigenvalues, the saddlepoint approximation
against Imhof's integral in mpmath); the set builders; and am.GWAS after its null-model part moved into am._null_model."""
import math

import mpmath
import numpy as np
import pytest
from scipy.special import chdtrc

import settest_truth as T
from eagleeverything_amd import am, r_api, rcpp_api
from test_lmm_host import HostSpectral

_ops = {}


def operands(name):
    if name not in _ops:
        _ops[name] = T.operands(name)
    return _ops[name]


def assert_meets_truth(name, res, say=None):
    """Every set of the panel: code, markers used, the degenerate markers exactly zero, and s, Phi, the seven statistics within
    settest_truth's bounds.  say: a callable that is shown the largest figure / bound ratio."""
    truth = T.golden(name)
    assert T.is_clear(name, truth), name                                   # the seed condition: 2^10 of margin at the degenerate threshold
    worst = 0.0
    for o, t in enumerate(truth):
        stat, info, s, Phi = res["stat"][o], res["info"][o], res["score"][o], res["cov"][o]
        assert info[0] == int(t["code"]) and info[1] == int(t["n_used"]), (name, o, info, t["code"], t["n_used"])
        deg = t["deg"] > 0.5
        assert (s[deg] == 0.0).all() and (Phi[deg, :] == 0.0).all() and (Phi[:, deg] == 0.0).all(), (name, o)
        assert np.array_equal(Phi, Phi.T), (name, o)
        for what, got, ref, b in (("s", s, t["s"], t["b_s"]), ("Phi", Phi, t["Phi"], t["b_Phi"])):
            err = np.abs(got - ref)
            assert (err <= b).all(), (name, o, what, float(np.max(err - b)), float(np.max(err)), float(np.max(b)))
            worst = max(worst, float(np.max(err[b > 0] / b[b > 0])) if (b > 0).any() else 0.0)
        if int(t["code"]) == 2:
            assert np.isnan(stat).all(), (name, o, stat)
            continue
        for k, what in enumerate(T.STATS):
            err = abs(stat[k] - t["stat"][k])
            assert err <= t["b_stat"][k], (name, o, what, stat[k], t["stat"][k], err, t["b_stat"][k])
            worst = max(worst, err / t["b_stat"][k])
    if say:
        say("%s: largest error / bound %.3g" % (name, worst))


@pytest.mark.parametrize("name", T.all_panels())
def test_host_meets_truth(name):
    lam, U, UtX, Uty, Z, Mt8, X, y, st, om = operands(name)
    res = r_api.settest_host(lam, UtX, Uty, Z, T.VAR_E, T.VAR_G, st, om)
    assert res["stat"].shape == (len(st), 7) and res["info"].shape == (len(st), 2) and res["info"].dtype == np.int32
    assert_meets_truth(name, res, print)


@pytest.mark.parametrize("name", T.small_panels())
def test_golden_entries_recomputed_live(name):
    """The stored truth is what settest_truth computes today, to within the bounds it hands out (the eigenbasis is made again here)."""
    live, gold = T.panel_truth(name), T.golden(name)
    assert len(live) == len(gold)
    for a, b in zip(live, gold):
        assert np.array_equal(a["deg"], b["deg"]) and a["code"] == b["code"] and a["n_used"] == b["n_used"]
        assert (np.abs(a["s"] - b["s"]) <= b["b_s"]).all() and (np.abs(a["Phi"] - b["Phi"]) <= b["b_Phi"]).all()
        if int(b["code"]) == 0:
            assert (np.abs(a["stat"] - b["stat"]) <= b["b_stat"]).all()
        for k in ("b_s", "b_Phi", "b_stat", "kappa"):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-6, atol=1e-300)


def host_scan(lam, UtX, Uty, Z, varE, varG):
    """a and vara of eagle_spectral_scan by its own formula (include/eagle_hip.h section 1d), in numpy."""
    d = 1.0 / (varE + varG * lam)
    A = UtX.T @ (d[:, None] * UtX)
    q = Z @ (d[:, None] * UtX)
    c1 = np.linalg.solve(A, UtX.T @ (d * Uty))
    return varG * (Z @ (d * Uty) - q @ c1), varG ** 2 * ((Z * Z) @ d - np.einsum("ij,ij->i", q, np.linalg.solve(A, q.T).T))


@pytest.mark.parametrize("name", ["n65", "m33", "c14"])
def test_scores_and_diagonal_are_the_scan(name):
    """s and diag Phi are the a and vara of the scan for the same operands, each within its bound of the truth; a set of one marker
    gives Q / Phi = a^2 / vara, so its burden p-value is the score test's."""
    lam, U, UtX, Uty, Z, Mt8, X, y, st, om = operands(name)
    a, vara = host_scan(lam, UtX, Uty, Z, T.VAR_E, T.VAR_G)
    t = T.golden(name)[0]                                                  # set 0 holds every marker of the panel, in order
    assert (np.abs(a - t["s"]) <= t["b_s"]).all() and (np.abs(vara - np.diag(t["Phi"])) <= np.diag(t["b_Phi"])).all()
    res = r_api.settest_host(lam, UtX, Uty, Z, T.VAR_E, T.VAR_G, st, om)
    assert (np.abs(res["score"][0] - a) <= 2 * t["b_s"]).all()
    assert (np.abs(np.diag(res["cov"][0]) - vara) <= 2 * np.diag(t["b_Phi"])).all()
    one = r_api.settest_host(lam, UtX, Uty, Z, T.VAR_E, T.VAR_G, [[j] for j in range(Z.shape[0])])
    Q, Ub, Vb, c1 = (one["stat"][:, k] for k in range(4))
    np.testing.assert_array_equal(Q, Ub * Ub)
    np.testing.assert_array_equal(Vb, c1)
    rel = 2 * (t["b_s"] / np.abs(t["s"]) + np.diag(t["b_Phi"]) / np.diag(t["Phi"]))      # of a^2 / vara, to first order
    score = a * a / vara
    assert (np.abs(Q / Vb - score) <= 2 * rel * score).all()
    p_set, p_score = chdtrc(1.0, Ub * Ub / Vb), chdtrc(1.0, score)
    # d log chdtrc(1, x) / d log x is at most x / 2 + 1 / 2 in magnitude
    assert (np.abs(p_set - p_score) <= 2 * rel * (score / 2 + 0.5) * p_score).all()


def test_refusals_of_the_restatement():
    lam, U, UtX, Uty, Z, *_ = operands("m2")
    ok = dict(lam=lam, UtX=UtX, Uty=Uty, Zrows=Z, varE=1.0, varG=1.0, sets=[[0, 1]], omega=None)
    for kw in (dict(sets=[[0, 2]]), dict(sets=[[]]), dict(sets=[list(range(65))]), dict(omega=[[1.0, -1.0]]), dict(omega=[[1.0, np.inf]]),
               dict(omega=[[1.0]]), dict(varG=-10.0), dict(UtX=np.ones((lam.size, 15))), dict(UtX=np.column_stack([UtX, UtX[:, 0]]))):
        with pytest.raises(ValueError):
            r_api.settest_host(**{**ok, **kw})
    res = r_api.settest_host(lam, UtX, Uty, Z, 1.0, 1.0, [[0, 1]], [[0.0, 0.0]])           # nothing left: code 2 and NaN
    assert res["info"][0, 0] == 2 and np.isnan(res["stat"]).all() and res["info"][0, 1] == 2


# ------------------------------------------------------------------------------------------------ p-values
@pytest.mark.parametrize("m,lam", [(1, 1.0), (5, 0.3), (16, 2.0 ** -7), (64, 3.7)])
def test_liu_is_chi_square_for_equal_eigenvalues(m, lam):
    for x in (0.5 * m, float(m), m + 6.0 * math.sqrt(2.0 * m), m + 15.0 * math.sqrt(2.0 * m)):
        ref = chdtrc(float(m), x)
        assert r_api.skat_pvalue(x * lam, eig=[lam] * m) == pytest.approx(ref, rel=1e-12)
        assert r_api.skat_pvalue(x * lam, c=[m * lam ** r for r in (1, 2, 3, 4)]) == pytest.approx(ref, rel=1e-12)
    with pytest.raises(ValueError):
        r_api.skat_pvalue(1.0)
    with pytest.raises(ValueError):
        r_api.skat_pvalue(1.0, c=[1.0, 1.0, 1.0, 1.0], method="saddle")
    with pytest.raises(ValueError):
        r_api.skat_pvalue(1.0, eig=[1.0], method="davies")


def imhof(vals, mult, x, dps=30, tol=1e-15):
    """P(sum_i lambda_i chi^2_1,i > x) by Imhof's (1961) integral 1/2 + 1/pi int_0^inf sin(theta(u)) / (u rho(u)) du, theta = 1/2 sum
    atan(lambda_i u) - x u / 2, rho = prod (1 + lambda_i^2 u^2)^(1/4), eigenvalue vals[i] with multiplicity mult[i]: cut where the tail's
    bound 2 / (m rho(U)) falls below tol, then 12-point Gauss-Legendre on every period of the fastest oscillation, at 30 digits."""
    from mpmath.calculus.quadrature import GaussLegendre
    with mpmath.workdps(dps):
        lm, x, q = [mpmath.mpf(v) for v in vals], mpmath.mpf(x), mpmath.mpf(1) / 4
        rho = lambda u: mpmath.fprod((1 + (l * u) ** 2) ** (q * k) for l, k in zip(lm, mult))
        f = lambda u: mpmath.sin(mpmath.fsum(k * mpmath.atan(l * u) for l, k in zip(lm, mult)) / 2 - x * u / 2) / (u * rho(u))
        U = mpmath.mpf(1)
        while 2 / (sum(mult) * rho(U)) > tol:
            U *= 1.25
        N = int(math.ceil(float(U) * (float(x) + sum(v * k for v, k in zip(vals, mult))) / (2 * math.pi))) + 1
        nodes = GaussLegendre(mpmath.mp).calc_nodes(3, mpmath.mp.prec)
        h, tot = U / N, mpmath.mpf(0)
        for k in range(N):
            mid = h * (k + mpmath.mpf(1) / 2)
            tot += mpmath.fsum(w * f(mid + h / 2 * t) for t, w in nodes)
        return float(mpmath.mpf(1) / 2 + tot * h / 2 / mpmath.pi)


SADDLE_CASES = [((1.0, 0.5, 0.25), (8, 8, 8), (27.2, 39.2, 50.2, 60.7, 68.6)),
                ((5.0, 0.5), (1, 23), (45.9, 86.1, 127.0, 168.0, 209.0))]
SADDLE_MEASURED = 0.0752


def test_saddlepoint_against_imhof():
    """Kuonen's saddlepoint p-value against Imhof's integral in mpmath at two fixed eigenvalue sets -- three levels of multiplicity 8,
    and one dominant eigenvalue over 23 equal ones -- with Q chosen so that p runs from 1e-2 to 1e-10.  Measured on the CPU: the largest
    relative deviation is 7.52 % (the dominant set at p = 3.5e-10; the deviations grow slowly into the tail: 2.1, 4.5, 5.9, 6.8, 7.5 %),
    0.41 % on the other set: the first-order Lugannani-Rice formula, whose relative error stays bounded where the Liu form is
    42 % and 72 % too small at those p.  Asserted: twice the measured value."""
    worst = 0.0
    for vals, mult, Qs in SADDLE_CASES:
        eig = np.repeat(vals, mult)
        ps = []
        for Q in Qs:
            ref = imhof(vals, mult, Q)
            got = r_api.skat_pvalue(Q, eig=eig, method="saddle")
            print("eig %s x %s  Q %.1f  imhof %.6e  saddle %.6e  rel %+.4f  liu rel %+.3f" % (vals, mult, Q, ref, got, got / ref - 1.0,
                                                                                        r_api.skat_pvalue(Q, eig=eig) / ref - 1.0))
            worst = max(worst, abs(got / ref - 1.0))
            ps.append(ref)
        assert 3e-3 < ps[0] < 3e-2 and 1e-10 < ps[-1] < 1e-9 and all(a > b for a, b in zip(ps, ps[1:]))
    print("largest relative deviation %.4f" % worst)
    assert worst <= 2 * SADDLE_MEASURED


def test_saddlepoint_lower_tail_and_centre():
    eig = [1.0, 0.5, 0.25, 0.1]
    rng = np.random.default_rng(5)
    x = (rng.chisquare(1, (400000, 4)) * eig).sum(axis=1)
    for Q in (0.2, 0.6, 4.0, 9.0):
        mc = float((x > Q).mean())
        assert r_api.skat_pvalue(Q, eig=eig, method="saddle") == pytest.approx(mc, abs=4 * math.sqrt(mc * (1 - mc) / x.size) + 0.1 * min(mc, 1 - mc))
    assert math.isnan(r_api.skat_pvalue(sum(eig), eig=eig, method="saddle")) and r_api.skat_pvalue(0.0, eig=eig, method="saddle") == 1.0
    assert r_api.skat_pvalue(4.0, eig=eig + [0.0, -1e-18], method="saddle") == r_api.skat_pvalue(4.0, eig=eig, method="saddle")


# ------------------------------------------------------------------------------------------------ the set builders
MAP3 = {"SNP": ["s%d" % j for j in range(150)], "Chr": ["1"] * 70 + ["2"] * 10 + ["X"] * 70,
        "Pos": list(range(1000, 71000, 1000)) + list(range(500, 10500, 1000)) + [10 * j for j in range(70)]}


def test_sets_from_windows():
    w = r_api.sets_from_windows(150, size=64)
    assert [s.size for s in w["sets"]] == [64, 64, 22] and w["names"][2] == "128-149" and np.array_equal(np.concatenate(w["sets"]), np.arange(150))
    w = r_api.sets_from_windows(MAP3, size=32)                              # cut at chromosome ends
    assert [(int(s[0]), int(s[-1])) for s in w["sets"]] == [(0, 31), (32, 63), (64, 69), (70, 79), (80, 111), (112, 143), (144, 149)]
    assert w["names"][3] == "2:70-79" and all(s.dtype == np.int64 for s in w["sets"])
    w = r_api.sets_from_windows(MAP3, size=8, step=4)                       # overlapping: a marker in two sets
    assert [(int(s[0]), int(s[-1])) for s in w["sets"][:3]] == [(0, 7), (4, 11), (8, 15)] and (int(w["sets"][16][0]), int(w["sets"][16][-1])) == (64, 69)
    assert (int(w["sets"][17][0]), int(w["sets"][17][-1])) == (70, 77) and (int(w["sets"][18][0]), int(w["sets"][18][-1])) == (74, 79)
    w = r_api.sets_from_windows({k: v[:80] for k, v in MAP3.items()}, kb=20)  # 20 kb windows from each chromosome's first marker
    assert [s.size for s in w["sets"]] == [20, 20, 20, 10, 10] and w["names"][0] == "1:1000-20999" and w["names"][4] == "2:500-20499"
    with pytest.raises(ValueError, match="X:0-19999"):                      # 70 markers within 700 bp
        r_api.sets_from_windows(MAP3, kb=20)
    for kw in (dict(), dict(size=8, kb=1), dict(size=65), dict(size=0), dict(size=4, step=0)):
        with pytest.raises(ValueError):
            r_api.sets_from_windows(MAP3, **kw)
    with pytest.raises(ValueError):
        r_api.sets_from_windows(150, kb=5)
    with pytest.raises(ValueError):
        r_api.sets_from_windows({"Chr": ["1", "1"], "Pos": [5, 3]}, kb=1)


def test_sets_from_table():
    t = r_api.sets_from_table(MAP3, [("geneA", "1", 5000, 9000), ("geneB", 2, 0, 2600), ("nothing", "1", 1, 10), ("geneC", "X", 100, 250)])
    assert t["names"] == ["geneA", "geneB", "geneC"] and t["empty"] == ["nothing"]
    assert [list(s) for s in t["sets"]] == [[4, 5, 6, 7, 8], [70, 71, 72], list(range(90, 106))]
    d = r_api.sets_from_table(MAP3, {"g": ("1", 1000, 64000)})
    assert d["sets"][0].size == 64
    with pytest.raises(ValueError, match=r"big1 \(65\).*big2 \(70\)"):
        r_api.sets_from_table(MAP3, [("ok", "1", 1000, 2000), ("big1", "1", 1000, 65000), ("big2", "X", 0, 10 ** 6)])
    with pytest.raises(ValueError):
        r_api.sets_from_table(MAP3, [("short", "1", 5)])
    with pytest.raises(ValueError):
        r_api.sets_from_table({"SNP": []}, [])


# ------------------------------------------------------------------------------------------------ am.GWAS after the refactor, am.SetTest
@pytest.fixture
def host_backend(monkeypatch):
    """The device calls of GWAS and SetTest replaced by their host restatements on lmm_truth's panel L129 (n = 67, 129 markers)."""
    import lmm_truth as LT
    G, Mt8, X, y, _ = LT.panel("L129")
    be = HostSpectral(Mt8)
    calls = []

    def scan(lam, UtX, Uty, varE, varG, n_markers, selected_loci=np.nan, device=0):
        a, vara = host_scan(lam, UtX, Uty, Mt8.astype(np.float64) @ be.U, varE, varG)
        return {"a": a.reshape(-1, 1), "vara": vara.reshape(-1, 1)}

    def lmm(lam, UtX, Uty, reml=True, theta0=0.0, tol=1e-10, max_iter=50, idx=None, n_markers=None, device=0):
        rows = np.arange(Mt8.shape[0]) if idx is None else np.asarray(idx)
        return r_api.lmm_host(lam, UtX, Uty, Mt8[rows].astype(np.float64) @ be.U, reml=reml, theta0=theta0, tol=tol, max_iter=max_iter)

    def settest(lam, UtX, Uty, varE, varG, sets, omega=None, scores=False, cov=False, device=0):
        calls.append((len(sets), cov))
        return r_api.settest_host(lam, UtX, Uty, Mt8.astype(np.float64) @ be.U, varE, varG, sets, omega)

    monkeypatch.setattr(rcpp_api, "spectral_scan", scan)
    monkeypatch.setattr(rcpp_api, "spectral_lmm", lmm)
    monkeypatch.setattr(rcpp_api, "spectral_settest", settest)
    monkeypatch.setattr(rcpp_api, "spectral_holds", lambda f, U, device=0: be.U is not None and U is be.U)
    geno = {"asciifileM": "M", "asciifileMt": "Mt", "dim_of_ascii_M": [Mt8.shape[1], Mt8.shape[0]]}
    return Mt8, X, y, geno, be, calls


def test_gwas_is_unchanged_by_the_shared_null_model(host_backend):
    """Every output of am.GWAS on a fixed seed against values computed by calling the pieces directly, with ==."""
    from scipy.special import chdtri, fdtrc
    Mt8, X, y, geno, be, _ = host_backend
    L, n = Mt8.shape
    for method in ("reml", "ml"):
        out = am.GWAS(y, X, geno, method=method, backend=be, map=["snp%d" % i for i in range(L)])
        assert be.calls == 1
        lam, U = be.eig
        UtX, Uty, Z = U.T @ X, U.T @ y, Mt8.astype(np.float64) @ U
        r0, m0 = am.emma_REMLE_eig(lam, UtX, Uty), am.emma_MLE_eig(lam, UtX, Uty)
        null_reml = {"delta": r0["delta"], "vg": r0["vg"], "ve": r0["ve"], "ll": r0["REML"]}
        null_ml = {"delta": m0["delta"], "vg": m0["vg"], "ve": m0["ve"], "ll": m0["ML"]}
        assert out["null_reml"] == null_reml and out["null"] == (null_reml if method == "reml" else null_ml)
        a, vara = host_scan(lam, UtX, Uty, Z, r0["ve"], r0["vg"])
        np.testing.assert_array_equal(out["score"], a * a / vara)
        np.testing.assert_array_equal(out["p_score"], chdtrc(1.0, a * a / vara))
        np.testing.assert_array_equal(out["beta_p3d"], r0["vg"] * a / vara)
        stat, info = r_api.lmm_host(lam, UtX, Uty, Z, reml=method == "reml", theta0=math.log((r0 if method == "reml" else m0)["delta"]))
        for j, k in enumerate(("beta", "se", "delta", "vg", "ll")):
            np.testing.assert_array_equal(out[k], stat[:, j])
        np.testing.assert_array_equal(out["ve"], stat[:, 2] * stat[:, 3])
        np.testing.assert_array_equal(out["code"], info[:, 0])
        np.testing.assert_array_equal(out["iterations"], info[:, 1])
        if method == "reml":
            np.testing.assert_array_equal(out["stat"], (stat[:, 0] / stat[:, 1]) ** 2)
            np.testing.assert_array_equal(out["p"], fdtrc(1.0, n - X.shape[1] - 1.0, out["stat"]))
        else:
            np.testing.assert_array_equal(out["stat"], np.maximum(2.0 * (stat[:, 4] - m0["ML"]), 0.0))
            np.testing.assert_array_equal(out["p"], chdtrc(1.0, out["stat"]))
        assert out["lambda_gc"] == float(np.nanmedian(a * a / vara) / chdtri(1.0, 0.5))
        assert out["n_used"] == n and out["method"] == method and len(out["indxNA"]) == 0 and out["names"][5] == "snp5"
        assert sorted(out) == sorted(["score", "p_score", "beta_p3d", "beta", "se", "stat", "p", "delta", "vg", "ve", "ll", "code", "iterations",
                                      "null", "null_reml", "lambda_gc", "n_used", "indxNA", "method", "names"])


def test_settest_bookkeeping_on_the_host(host_backend):
    Mt8, X, y, geno, be, calls = host_backend
    L, n = Mt8.shape
    am.GWAS(y, X, geno, exact="none", backend=be)
    win = r_api.sets_from_windows(L, size=16)
    out = r_api.SetTest(y, X, geno, win, backend=be, p_refine=0.2, map=["snp%d" % i for i in range(L)])
    assert be.calls == 1                                                   # the backend GWAS ran on rebuilds nothing
    k = len(win["sets"])
    lam, U = be.eig
    UtX, Uty = U.T @ X, U.T @ y
    r0 = am.emma_REMLE_eig(lam, UtX, Uty)
    assert out["null"] == {"delta": r0["delta"], "vg": r0["vg"], "ve": r0["ve"], "ll": r0["REML"]}
    h = r_api.settest_host(lam, UtX, Uty, Mt8.astype(np.float64) @ U, r0["ve"], r0["vg"], win["sets"])
    Q, Ub, Vb = (h["stat"][:, j] for j in range(3))
    np.testing.assert_array_equal(out["Q"], Q)
    np.testing.assert_array_equal(out["burden"], Ub * Ub / Vb)
    np.testing.assert_array_equal(out["p_burden"], chdtrc(1.0, Ub * Ub / Vb))
    np.testing.assert_array_equal(out["beta_burden"], r0["vg"] * Ub / Vb)
    liu = np.array([r_api.skat_pvalue(Q[o], c=h["stat"][o, 3:7]) for o in range(k)])
    np.testing.assert_array_equal(out["p_skat_liu"], liu)
    hit = liu < 0.2
    assert 0 < hit.sum() < k and np.array_equal(out["refined"], hit) and calls == [(k, False), (int(hit.sum()), True)]
    for o in range(k):
        ref = r_api.skat_pvalue(Q[o], eig=np.linalg.eigvalsh(h["cov"][o]), method="saddle") if hit[o] else liu[o]
        assert out["p_skat"][o] == ref
    assert list(out["n_markers"]) == [16] * 8 + [1] and list(out["n_used"]) == list(h["info"][:, 1]) and (out["code"] == 0).all()
    assert out["names"] == win["names"] and out["markers"][8] == ["snp128"] and out["n_used_individuals"] == n
    # weights: one per marker of the panel; the planted marker 0 (lmm_truth's panel) makes its window the smallest p
    w = np.linspace(0.5, 2.0, L)
    outw = am.SetTest(y, X, geno, win["sets"], weights=w, backend=be, p_refine=None)
    hw = r_api.settest_host(lam, UtX, Uty, Mt8.astype(np.float64) @ U, r0["ve"], r0["vg"], win["sets"], [w[s] for s in win["sets"]])
    np.testing.assert_array_equal(outw["Q"], hw["stat"][:, 0])
    assert not outw["refined"].any() and outw["names"][0] == "set1" and "markers" not in outw
    with pytest.raises(NotImplementedError, match="Zmat"):
        am.SetTest(y, X, geno, win, backend=be, Zmat=np.eye(3))
    for kw in (dict(sets=[list(range(65))]), dict(sets=[[]]), dict(sets=[[0, L]]), dict(weights="maf"), dict(weights=np.ones(L - 1)),
               dict(weights=-np.ones(L)), dict(p_refine=2.0), dict(weights=("beta", 0.0, 1.0))):
        with pytest.raises(ValueError):
            am.SetTest(**{**dict(trait=y, X=X, geno=geno, sets=win["sets"], backend=be), **kw})
    with pytest.raises(TypeError):
        am.SetTest(y, X, geno, win, backend=object())


def test_beta_weights_are_the_density_of_the_maf(host_backend, monkeypatch):
    """weights="beta" / ("beta", a, b): Beta(MAF; a, b) of r_api.MarkerStats per marker, 0 where the MAF is NaN (no called genotype) or
    the density is not finite (MAF = 0 with a < 1); the weights that reach the device call are those of each set's markers."""
    from scipy.stats import beta
    Mt8, X, y, geno, be, calls = host_backend
    L, n = Mt8.shape
    maf = np.minimum((Mt8 + 1).sum(axis=1), 2 * n - (Mt8 + 1).sum(axis=1)) / (2.0 * n)
    maf[5], maf[6] = np.nan, 0.0
    asked = []
    monkeypatch.setattr(r_api, "MarkerStats", lambda g, **kw: (asked.append(g["asciifileMt"]), {"maf": maf.copy()})[1])
    seen = []
    real = rcpp_api.spectral_settest
    monkeypatch.setattr(rcpp_api, "spectral_settest", lambda *a, **k: (seen.append([np.array(w) for w in a[6]]), real(*a, **k))[1])
    sets = [np.arange(0, 16), np.array([40, 3, 6, 5])]
    for spec, (a, b) in (("beta", (1.0, 25.0)), (("beta",), (1.0, 25.0)), (("beta", 0.5, 0.5), (0.5, 0.5)), (("beta", 2.0, 3.0), (2.0, 3.0))):
        out = am.SetTest(y, X, geno, sets, weights=spec, backend=be, p_refine=None)
        want = beta.pdf(np.where(np.isnan(maf), 0.0, maf), a, b)
        want[5] = 0.0
        if not np.isfinite(want[6]):
            want[6] = 0.0                                                  # Beta(0; 1/2, 1/2) is infinite
        assert np.isfinite(want).all() and (want >= 0).all() and want[6] == (25.0 if (a, b) == (1.0, 25.0) else 0.0)
        for w, s in zip(seen[-1], sets):
            np.testing.assert_array_equal(w, want[s])
        lam, U = be.eig
        h = r_api.settest_host(lam, U.T @ X, U.T @ y, Mt8.astype(np.float64) @ U, out["null"]["ve"], out["null"]["vg"], sets, [want[s] for s in sets])
        np.testing.assert_array_equal(out["Q"], h["stat"][:, 0])
    assert asked == ["Mt"] * 4
    assert want[3] == pytest.approx(12.0 * maf[3] * (1.0 - maf[3]) ** 2, rel=1e-12)     # Beta(x; 2, 3) = 12 x (1 - x)^2
