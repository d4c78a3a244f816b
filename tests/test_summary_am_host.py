"""SummaryAM (r_api.SummaryAM, am.SummaryAM_traits) on the host, MM^T from the C oracle.

The yardstick is `straight_summary` below: summary_am.R:123-215 restated literally -- emma.REMLE / emma.MLE with their n x n
eigen() calls (am.emma_REMLE / am.emma_MLE), solve(H), K'' = K/max(K) + 0.05 I.  The code under test works in the eigenbasis of
K and never calls it."""
import math

import numpy as np
import pytest
from scipy.stats import chi2

from eagleeverything_amd import am, host_model, r_api, synth

from test_am_driver import OracleBackend

QTL = [300, 1500, 2700, 4200]


def straight_summary(y, baseX, Msel, K):
    """summary_am.R:142-211 as the reference computes it, n x n throughout."""
    n, q = baseX.shape
    F = np.column_stack([baseX, Msel])
    eR = am.emma_REMLE(y, F, K, llim=-100, ulim=100)
    H = eR["vg"] * K + eR["ve"] * np.eye(n)
    Hinv = np.linalg.solve(H, np.eye(n))
    Ainv = np.linalg.solve(F.T @ Hinv @ F, np.eye(F.shape[1]))
    beta = Ainv @ F.T @ Hinv @ y
    W = beta ** 2 / np.diag(Ainv)
    pval = 1 - chi2.cdf(W, 1)
    K2 = K / K.max() + 0.05 * np.eye(n)
    base = am.emma_MLE(y, baseX, K2, llim=-100, ulim=100)["ML"]
    rsq = [1 - math.exp(-2 / n * (am.emma_MLE(y, F[:, :q + k], K2, llim=-100, ulim=100)["ML"] - base))
           for k in range(1, Msel.shape[1] + 1)]
    return {"estimate": beta, "W": W, "p_value": pval, "Rsq": np.array(rsq)}


class FileBackend(OracleBackend):
    """The oracle backend with AM()'s NA reshape in FILES mode (VIEW needs a device)."""

    def reshape(self, geno, indxNA):
        return am.reshape_geno(geno, indxNA)


class CountingLA:
    """host_model.algebra() with its eigh calls counted."""

    def __init__(self, la):
        self.la, self.eighs = la, 0

    def eigh(self, A):
        self.eighs += 1
        return self.la.eigh(A)

    def __getattr__(self, name):
        return getattr(self.la, name)


def planted(g, seed=1):
    rng = np.random.default_rng(seed)
    Mt8 = np.ascontiguousarray(g["M8"].T)
    y = g["X"] @ [1.0, 0.3, -0.2] + Mt8[QTL].T.astype(float) @ [1.5, -1.2, 1.0, 0.8] + 0.6 * rng.standard_normal(Mt8.shape[1])
    return Mt8, y


def assert_matches_straight(got, ref):
    np.testing.assert_allclose(got["size"]["estimate"], ref["estimate"], rtol=1e-8)
    np.testing.assert_allclose(got["pvalue"]["W"], ref["W"], rtol=1e-8)
    np.testing.assert_allclose(got["R"]["Prop_var_explained"], ref["Rsq"], rtol=1e-8)
    p, pr = np.array(got["pvalue"]["p_value"]), ref["p_value"]
    ok = pr > 1e-300
    np.testing.assert_allclose(p[ok], pr[ok], rtol=1e-8)
    assert np.all(p[~ok] <= 1e-300)
    assert got["size"]["p_value"] == got["pvalue"]["p_value"]


def assert_same_tables(a, b, rtol):
    assert a["pvalue"]["effects"] == b["pvalue"]["effects"] and a["R"]["Marker_name"] == b["R"]["Marker_name"]
    for part, key in (("size", "estimate"), ("pvalue", "W"), ("pvalue", "p_value"), ("R", "Prop_var_explained")):
        np.testing.assert_allclose(a[part][key], b[part][key], rtol=rtol, atol=0, err_msg=key)


def oracle_K(oracle, geno):
    return OracleBackend(oracle).calcMMt(geno, 8, 1, np.array([np.nan]), True)


def test_summary_am_matches_straight_restatement_cpu(oracle, golden, tmp_path):
    g = golden("genoDemo_150x4998")
    Mt8, y = planted(g)
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    ob = FileBackend(oracle)
    res = am.AM(y, g["X"], geno, maxit=8, backend=ob)
    picks = res["selected_loci"]
    assert len(picks) >= 3
    msgs = []
    got = r_api.SummaryAM(res, y, g["X"], geno, backend=ob, message=msgs.append)
    ref = straight_summary(y, g["X"], Mt8[np.array(picks) - 1].T.astype(float), oracle_K(oracle, geno))
    assert_matches_straight(got, ref)
    names = ["intercept", "X2", "X3"] + ["M%d" % j for j in picks]
    assert got["pvalue"]["effects"] == names and got["size"]["effect_names"] == names
    assert got["R"]["Marker_name"] == ["+ M%d" % j for j in picks]
    assert "     Size and Significance of Effects in Final Model    \n" in msgs
    assert "%15s  %10f         %.3E\n" % ("M%d" % picks[0], ref["estimate"][3], ref["p_value"][3]) in msgs
    assert "  %+15s          %.3f\n" % ("+  M%d" % picks[-1], ref["Rsq"][-1]) in msgs
    # a map and X names are used for reporting only
    snp = ["snp_%d" % j for j in range(1, Mt8.shape[0] + 1)]
    named = r_api.SummaryAM(res, y, g["X"], geno, map={"SNP": snp}, xnames=["mu", "a", "b"], backend=ob)
    assert named["pvalue"]["effects"] == ["mu", "a", "b"] + ["snp_%d" % j for j in picks]
    assert named["R"]["Marker_name"] == ["+ snp_%d" % j for j in picks]
    assert_same_tables(named | {"pvalue": dict(named["pvalue"], effects=names), "R": dict(named["R"], Marker_name=got["R"]["Marker_name"])},
                       got, rtol=0)


def test_summary_am_drops_na_rows_like_reshaped_files_cpu(oracle, golden, tmp_path):
    g = golden("genoDemo_150x4998")
    Mt8, y = planted(g, seed=2)
    X = g["X"].copy()
    y[[7, 64]] = np.nan
    X[101, 2] = np.nan
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    ob = FileBackend(oracle)
    res = am.AM(y, X, geno, maxit=8, backend=ob)
    assert list(res["indxNA"]) == [102, 65, 8] and len(res["selected_loci"]) >= 3
    got = r_api.SummaryAM(res, y, X, geno, backend=ob)
    keep = np.ones(y.size, dtype=bool)
    keep[[7, 64, 101]] = False
    geno_r = am.reshape_geno(geno, res["indxNA"])                       # FILES mode: M.asciitmp / Mt.asciitmp
    assert geno_r["dim_of_ascii_M"] == [147, Mt8.shape[0]]
    plain = r_api.SummaryAM(dict(res, indxNA=np.array([], dtype=np.int64)), y[keep], X[keep], geno_r, backend=OracleBackend(oracle))
    assert_same_tables(got, plain, rtol=1e-12)
    Msel = Mt8[np.array(res["selected_loci"]) - 1][:, keep].T.astype(float)
    assert_matches_straight(got, straight_summary(y[keep], X[keep], Msel, oracle_K(oracle, geno_r)))


def test_summary_am_empty_model_returns_none():
    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("backend used for an empty model")
    msgs = []
    out = r_api.SummaryAM({"selected_loci": [], "indxNA": np.array([], dtype=np.int64)}, np.zeros(5), np.ones((5, 1)),
                          {"asciifileM": "/nonexistent", "asciifileMt": "/nonexistent", "dim_of_ascii_M": [5, 9]},
                          backend=NoCalls(), message=msgs.append)
    assert out is None
    assert msgs == [" No significant marker-trait associations have been found by AM. \n", " Nothing to summarize. \n"]
    assert am.SummaryAM_traits([{"selected_loci": []}], np.zeros((5, 1)), np.ones((5, 1)), None, backend=NoCalls()) == [None]


def test_summary_am_with_eig_calls_no_eigh(oracle, golden, tmp_path, monkeypatch):
    g = golden("genoDemo_150x4998")
    Mt8, y = planted(g)
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    ob = FileBackend(oracle)
    res = am.AM(y, g["X"], geno, maxit=8, backend=ob)
    eig = np.linalg.eigh(oracle_K(oracle, geno))
    la = CountingLA(host_model.algebra())
    monkeypatch.setattr(host_model, "_la", la)
    with_eig = r_api.SummaryAM(res, y, g["X"], geno, backend=ob, eig=eig)
    assert la.eighs == 0
    fresh = r_api.SummaryAM(res, y, g["X"], geno, backend=ob)
    assert la.eighs == 1
    assert_same_tables(with_eig, fresh, rtol=1e-10)
    with pytest.raises(ValueError, match="eig"):
        r_api.SummaryAM(res, y, g["X"], geno, backend=ob, eig=(eig[0][:-1], eig[1][:-1, :-1]))


def test_summary_am_traits_equals_per_trait_summary_cpu(oracle, golden, tmp_path, monkeypatch):
    g = golden("genoDemo_150x4998")
    Mt8, y = planted(g)
    rng = np.random.default_rng(5)
    M = Mt8.T.astype(float)
    Y = np.column_stack([y] + [g["X"] @ [0.5, 0.0, 0.1] + M[:, qs] @ b + 0.6 * rng.standard_normal(150)
                               for qs, b in (([100, 2000, 3500], [1.2, 1.0, -1.1]), ([700, 2900, 4600], [-1.4, 1.0, 0.9]),
                                             ([300, 1200, 3100], [1.0, 1.3, -1.0]))])
    Y[[4, 40], 1] = np.nan
    Y[120, 3] = np.nan
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    ob = FileBackend(oracle)
    union = np.isnan(Y).any(axis=1)
    results = []
    for t in range(Y.shape[1]):
        yt = Y[:, t].copy()
        yt[union] = np.nan
        results.append(am.AM(yt, g["X"], geno, maxit=6, backend=ob))
    assert all(r["selected_loci"] for r in results) and len({tuple(r["selected_loci"]) for r in results}) == len(results)
    singles = [r_api.SummaryAM(r, Y[:, t], g["X"], geno, backend=ob) for t, r in enumerate(results)]
    la = CountingLA(host_model.algebra())
    monkeypatch.setattr(host_model, "_la", la)
    many = am.SummaryAM_traits(results, Y, g["X"], geno, backend=ob)
    assert la.eighs == 1
    assert len(many) == Y.shape[1]
    for a, b in zip(many, singles):
        assert_same_tables(a, b, rtol=1e-10)
    # a trait without picks gets None among the others
    mixed = am.SummaryAM_traits([results[0], dict(results[1], selected_loci=[])] + results[2:], Y, g["X"], geno, backend=ob)
    assert mixed[1] is None
    for t in (0, 2, 3):
        assert_same_tables(mixed[t], singles[t], rtol=1e-10)
