"""FPR4AM on the host: the two rules that turn gamma_star into a gamma, the weight gamma in extBIC and in
the AM() loops, the batched EMMA in the eigenbasis against the per-trait functions it batches, and FPR4AM itself with a numpy
stand-in for the spectral calls against the loop it stands for, AM(y[pi_r], X, geno, maxit=2) on the oracle backend."""
import math

import numpy as np
import pytest

from eagleeverything_amd import am, host_model, r_api, rcpp_api, synth

from test_am_driver import OracleBackend
from test_repeated_measures_host import NumpyBackend, rm_fixture
from test_traits_host import _HostSpectral


# ------------------------------------------------------------------------------------------------------ the two rules
def test_fpr_curve_counts_strictly_larger_thresholds():
    gs = np.array([0.5, -1.0, 0.5, 2.0, 0.0])
    np.testing.assert_array_equal(am.fpr_curve(gs, [-2.0, -1.0, 0.0, 0.25, 0.5, 1.0, 2.0, 3.0]),
                                  np.array([5, 4, 3, 3, 1, 1, 0, 0]) / 5)
    f = am.fpr_curve(gs, np.linspace(-2, 3, 101))
    assert np.all(np.diff(f) <= 0)                                    # never increases


def test_choose_gamma_is_the_kth_largest_clipped_at_zero():
    gs = np.array([0.9, 0.1, 0.4, 0.7, 0.3, 0.8, 0.2, 0.6, 0.5, 1.3])   # R = 10, distinct
    srt = np.sort(gs)[::-1]
    assert am.choose_gamma(gs, 0.2) == srt[2]                         # 0.2 * 10 integral: k = 3
    assert am.choose_gamma(gs, 0.25) == srt[2]                        # not integral: floor(2.5) + 1 = 3
    assert am.choose_gamma(gs, 0.05) == srt[0] == 1.3                 # k = 1: the largest, above 1 and not snapped
    assert am.choose_gamma(gs, 0.99) == srt[9]
    assert am.choose_gamma(-gs, 0.3) == 0.0                           # all negative: gamma = 0 already meets any rate
    assert am.choose_gamma(np.array([-0.5, 0.2, -0.1, -3.0]), 0.25) == 0.0   # 2nd largest is negative
    ties = np.array([0.7, 0.7, 0.7, 0.2, 0.2, 0.1, 0.9, 0.7])
    assert am.choose_gamma(ties, 0.25) == 0.7                         # k = 3 falls into the tie; FPR(0.7) = 1/8
    assert am.fpr_curve(ties, 0.7)[0] == 1 / 8
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            am.choose_gamma(gs, bad)


@pytest.mark.parametrize("R", [7, 10, 64, 100, 400])
def test_choose_gamma_is_the_smallest_gamma_that_meets_the_rate(R):
    rng = np.random.default_rng(R)
    gs = np.round(rng.normal(0.6, 0.5, R), 1)                         # rounded: many ties
    for fpr in (0.01, 0.05, 0.07, 0.1, 0.25, 0.29, 0.5, 0.57, 0.9):
        g = am.choose_gamma(gs, fpr)
        k = math.floor(fpr * R + 1e-9) + 1                            # the rule of section 4.7d, the product's rounding aside
        assert g == max(np.sort(gs)[::-1][k - 1], 0.0), (R, fpr)
        assert am.fpr_curve(gs, g)[0] <= fpr
        if g > 0:
            assert am.fpr_curve(gs, g - 1e-9)[0] > fpr, (R, fpr)


# ------------------------------------------------------------------------------------------------------ gamma in extBIC and AM
def test_calc_extBIC_gamma_weights_the_lchoose_term_only(golden):
    g = golden("geno_150x100")
    K = g["MMt"] / g["MMt_norm_max"] + 0.95 * np.eye(150)
    M = g["M8"].astype(np.float64)
    L = 4998
    for X in (g["X"], np.column_stack([g["X"], M[:, [3, 50]]])):
        base = am.calc_extBIC(g["y"], X, K, L)
        assert am.calc_extBIC(g["y"], X, K, L, gamma=1.0) == base     # bit for bit
        for gam in (0.0, 0.3, 0.999, 1.7):
            want = base - 2 * (1 - gam) * am._lchoose(L, X.shape[1] - 1)
            assert am.calc_extBIC(g["y"], X, K, L, gamma=gam) == pytest.approx(want, rel=1e-12, abs=0.0)


class PlainNumpyBackend(NumpyBackend):
    """NumpyBackend for AM() without Zmat: the scan of the model with Z = I."""

    def find_qtl(self, geno, MMt, best_ve, best_vg, currentX, trait, **kw):
        zm = host_model.ZModel(MMt, np.arange(MMt.shape[0]))
        return super().find_qtl(geno, MMt, best_ve, best_vg, currentX, trait, Zmat=zm)


def _same_dict(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _rm_case(golden):
    M, ind, y, X, planted = rm_fixture(golden)
    return M, ind, y, X, planted, {"M": M, "dim_of_ascii_M": list(M.shape)}


def test_AM_gamma_one_is_AM_on_both_paths(golden):
    M, ind, y, X, planted, geno = _rm_case(golden)
    _same_dict(am.AM(y, X, geno, maxit=6, backend=NumpyBackend(M), Zmat=ind),
               am.AM(y, X, geno, maxit=6, backend=NumpyBackend(M), Zmat=ind, gamma=1.0))
    # the plain path: one record per individual (the first of each), the individuals without one as NaN rows
    first = np.full(M.shape[0], -1)
    first[ind[::-1]] = np.arange(ind.size)[::-1]
    y1 = np.where(first >= 0, y[first], np.nan)
    X1 = X[np.maximum(first, 0)]
    ref = am.AM(y1, X1, geno, maxit=6, backend=PlainNumpyBackend(M))
    _same_dict(ref, am.AM(y1, X1, geno, maxit=6, backend=PlainNumpyBackend(M), gamma=1.0))
    assert len(ref["all_picks"]) >= 1 and ref["indxNA"].size == 2


def test_a_smaller_gamma_never_selects_fewer_loci(golden):
    M, ind, y, X, planted, geno = _rm_case(golden)
    prev = None
    for gam in (1.5, 1.0, 0.6, 0.3, 0.0):
        res = am.AM(y, X, geno, maxit=12, backend=NumpyBackend(M), Zmat=ind, gamma=gam)
        sel = res["selected_loci"]
        if prev is not None:
            assert len(sel) >= len(prev) and sel[:len(prev)] == prev, gam   # the same path, stopped later
        prev = sel
    assert set(p + 1 for p in planted) <= set(prev)


# ------------------------------------------------------------------------------------------------------ batched EMMA
def _panel_traits(golden, name, T, cov, seed=5):
    """T traits on a golden panel: permutations of its y, and from the 4th on every third one white noise scaled up (vg -> 0)."""
    g = golden(name)
    n = g["y"].size
    K = g["MMt"] / g["MMt_norm_max"] + 0.95 * np.eye(n)
    lam, U = np.linalg.eigh(K)
    rng = np.random.default_rng(seed)
    cols = [g["y"]] + [g["y"][rng.permutation(n)] for _ in range(T - 1)]
    for t in range(3, T, 3):
        cols[t] = 5.0 * rng.standard_normal(n)
    X = g["X"] if cov else np.ones((n, 1))
    return g, lam, U, X, np.column_stack(cols)


@pytest.mark.parametrize("cov", [False, True])
@pytest.mark.parametrize("T", [1, 7, 40])
@pytest.mark.parametrize("name", ["geno_150x100", "genoDemo_150x4998"])
def test_batched_emma_equals_the_per_trait_emma(golden, name, T, cov):
    g, lam, U, X, Y = _panel_traits(golden, name, T, cov)
    UtX, UtY = U.T @ X, U.T @ Y
    last = U.T @ g["M8"][:, (7 + 13 * np.arange(T)) % g["M8"].shape[1]].astype(np.float64)   # a marker column per trait: the pick
    ends = set()
    for lst in (None, last):
        for lims in ({}, {"llim": -100, "ulim": 100}):
            br = am.emma_REMLE_eig_batch(lam, UtX, UtY, last=lst, **lims)
            bm = am.emma_MLE_eig_batch(lam, UtX, UtY, last=lst, **lims)
            for k in ("REML", "delta", "ve", "vg"):
                assert br[k].shape == (T,)
            for t in range(T):
                Xt = UtX if lst is None else np.column_stack([UtX, lst[:, t]])
                r1 = am.emma_REMLE_eig(lam, Xt, UtY[:, t], **lims)
                m1 = am.emma_MLE_eig(lam, Xt, UtY[:, t], **lims)
                np.testing.assert_allclose(br["REML"][t], r1["REML"], rtol=1e-8)
                np.testing.assert_allclose(bm["ML"][t], m1["ML"], rtol=1e-8)
                for got, ref in ((br, r1), (bm, m1)):
                    np.testing.assert_allclose([got["ve"][t], got["vg"][t]], [ref["ve"], ref["vg"]], rtol=1e-6)
                    assert (got["delta"][t] in (math.exp(-10), math.exp(10), math.exp(-100), math.exp(100))) == \
                           (ref["delta"] in (math.exp(-10), math.exp(10), math.exp(-100), math.exp(100))), t
                    if ref["delta"] >= math.exp(10):
                        assert got["delta"][t] == ref["delta"]          # the same end point: vg -> 0
                        ends.add(t)
    if T >= 7:
        assert ends, "no trait of this case ends at the upper limit of delta (vg -> 0)"


def test_batched_emma_singular_design_and_bad_shapes(golden):
    g, lam, U, X, Y = _panel_traits(golden, "geno_150x100", 3, True)
    UtX, UtY = U.T @ X, U.T @ Y
    last = np.column_stack([UtX[:, 1], U.T @ g["M8"][:, 5].astype(np.float64), UtX[:, 2]])       # traits 0 and 2: a duplicated column
    r = am.emma_MLE_eig_batch(lam, UtX, UtY, last=last)
    for t in range(3):
        one = am.emma_MLE_eig(lam, np.column_stack([UtX, last[:, t]]), UtY[:, t])
        assert (r["ML"][t] == 0) == (one["ML"] == 0)
        np.testing.assert_allclose(r["ML"][t], one["ML"], rtol=1e-8)
    assert r["ML"][1] != 0
    with pytest.raises(ValueError):
        am.emma_MLE_eig_batch(lam, UtX, UtY, last=last[:, :2])


def test_batched_emma_grid_is_one_product_through_the_algebra(golden, monkeypatch):
    g, lam, U, X, Y = _panel_traits(golden, "geno_150x100", 7, True)
    calls = []

    class LA:
        name = "host"

        @staticmethod
        def mm(A, B):
            calls.append((A.shape, B.shape))
            return A @ B

    monkeypatch.setattr(host_model, "_la", LA())
    am.emma_REMLE_eig_batch(lam, U.T @ X, U.T @ Y)
    assert calls == [((7 * 10, 150), (150, 202))]                     # T (q+1)(q+2)/2 stacked products against [W | W^2]


# ------------------------------------------------------------------------------------------------------ FPR4AM on the host
def _host_fpr(oracle, monkeypatch):
    ob = OracleBackend(oracle)
    fake = _HostSpectral()
    held = {}

    def prepare(f_name_ascii, dims, U, max_memory_in_Gbytes=8.0, device=0):
        fake.prepare(f_name_ascii, dims, U)
        held["key"] = (str(f_name_ascii), np.array(U, copy=True))
        held["prepares"] = held.get("prepares", 0) + 1

    monkeypatch.setattr(r_api, "calcMMt", lambda geno, availmemGb, ncpu, sel, quiet, device=0: ob.calcMMt(geno, availmemGb, ncpu, sel, quiet))
    monkeypatch.setattr(rcpp_api, "spectral_prepare", prepare)
    monkeypatch.setattr(rcpp_api, "spectral_holds", lambda f, U, device=0: "key" in held and held["key"][0] == str(f)
                        and np.array_equal(held["key"][1], U))
    monkeypatch.setattr(rcpp_api, "spectral_scan_traits", fake.scan)
    monkeypatch.setattr(rcpp_api, "spectral_rows", fake.rows)
    file_reshape = am.reshape_geno
    monkeypatch.setattr(am, "reshape_geno", lambda geno, indxNA, view=False, device=0: file_reshape(geno, indxNA))
    return ob, fake, held


@pytest.mark.parametrize("cov,nan_rows", [(True, ()), (False, (3, 77, 149))])
def test_FPR4AM_is_the_AM_loop_on_permuted_traits_cpu(oracle, golden, tmp_path, monkeypatch, cov, nan_rows):
    g = golden("geno_150x100")
    geno = synth.write_geno_pair(str(tmp_path), np.ascontiguousarray(g["M8"].T))
    ob, fake, held = _host_fpr(oracle, monkeypatch)
    y = g["y"].copy()
    y[list(nan_rows)] = np.nan
    X = g["X"] if cov else np.ones((150, 1))
    R, seed = 12, 7
    res = am.FPR4AM(y, X, geno, falseposrate=0.1, numreps=R, seed=seed)
    assert res["numreps"] == R and res["seed"] == seed
    np.testing.assert_array_equal(res["indxNA"], np.array(sorted(nan_rows, reverse=True), dtype=np.int64) + 1)
    keep = ~np.isnan(y)
    yk, Xk = y[keep], X[keep]
    n, L = yk.size, 100
    rgeno = am.reshape_geno(geno, res["indxNA"]) if nan_rows else geno
    rng = np.random.default_rng(seed)
    q = X.shape[1]
    c = am._lchoose(L, q) - am._lchoose(L, q - 1)
    for r in range(R):
        ref = am.AM(yk[rng.permutation(n)], Xk, rgeno, maxit=2, backend=ob)
        assert ref["all_picks"][0] == res["picks"][r], r
        tr = ref["extBIC_trace"]
        np.testing.assert_allclose(-2 * res["ML0"][r] + (q + 1) * math.log(n) + 2 * am._lchoose(L, q - 1), tr[0], rtol=1e-8)
        np.testing.assert_allclose(-2 * res["ML1"][r] + (q + 2) * math.log(n) + 2 * am._lchoose(L, q), tr[1], rtol=1e-8)
        assert (tr[1] < tr[0]) == (1 < res["gamma_star"][r]), r
        assert res["gamma_star"][r] == (2 * (res["ML1"][r] - res["ML0"][r]) - math.log(n)) / (2 * c)
    assert res["setgamma"] == am.choose_gamma(res["gamma_star"], 0.1)
    assert res["falseposrate"] == am.fpr_curve(res["gamma_star"], res["setgamma"])[0] <= 0.1


def test_FPR4AM_chunks_seed_and_eig_reuse_cpu(oracle, golden, tmp_path, monkeypatch):
    g = golden("geno_150x100")
    geno = synth.write_geno_pair(str(tmp_path), np.ascontiguousarray(g["M8"].T))
    ob, fake, held = _host_fpr(oracle, monkeypatch)
    a = am.FPR4AM(g["y"], g["X"], geno, numreps=17, seed=3)
    assert held["prepares"] == 1 and fake.calls == 1                  # default chunk: one batched scan call for 17 permutations
    b = am.FPR4AM(g["y"], g["X"], geno, numreps=17, seed=3)
    assert held["prepares"] == 1                                      # the same Z is still resident: no second prepare
    c5 = am.FPR4AM(g["y"], g["X"], geno, numreps=17, seed=3, chunk=5)
    assert fake.calls == 1 + 1 + 4
    K = ob.calcMMt(geno, 8, 1, np.array([np.nan]), True)
    lam, U = np.linalg.eigh(K)
    monkeypatch.setattr(r_api, "calcMMt", lambda *a, **k: pytest.fail("eig= given: no calcMMt"))
    monkeypatch.setattr(host_model._la, "eigh", lambda *a: pytest.fail("eig= given: no eigh"), raising=False)
    e = am.FPR4AM(g["y"], g["X"], geno, numreps=17, seed=3, eig=(lam, U))
    for other in (b, c5, e):
        for k in a:
            np.testing.assert_array_equal(a[k], other[k], err_msg=k)
    d = am.FPR4AM(g["y"], g["X"], geno, numreps=17, seed=4, eig=(lam, U))
    assert not np.array_equal(a["gamma_star"], d["gamma_star"])
    assert r_api.FPR4AM is not None and r_api.FPR4AM(g["y"], g["X"], geno, numreps=3, seed=3, eig=(lam, U))["numreps"] == 3


def test_FPR4AM_argument_checks_come_before_any_device_work():
    geno = {"asciifileM": "/nonexistent/M", "asciifileMt": "/nonexistent/Mt", "dim_of_ascii_M": (150, 4998)}
    y, X = np.zeros(150), np.ones((150, 1))
    for kw in ({"falseposrate": 0.0}, {"falseposrate": 1.0}, {"numreps": 0}, {"chunk": 0}):
        with pytest.raises(ValueError):
            am.FPR4AM(y, X, geno, **kw)
    with pytest.raises(ValueError, match="30"):
        am.FPR4AM(y, np.ones((150, 31)), geno)
    with pytest.raises(TypeError):
        am.FPR4AM(y, X, geno, Zmat=np.arange(150))
