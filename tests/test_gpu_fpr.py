"""FPR4AM on an MI355X against the loop it stands for, AM(y[pi_r], X, geno, maxit=2) with the
SpectralBackend and pi_r regenerated from the seed; its invariances (seed, chunk, eig=, two sub-contexts on one card); a hold-out
check of the calibrated rate; and a planted panel on which the calibrated gamma must not lose a locus gamma = 1 finds.

Seeds.  The golden panels hold duplicated markers, so some permutations have an exact tie at the top of tsq.  The seeds of the
comparison with the loop (3 on 150 x 100, 9 on 150 x 4998) were chosen, with a numpy scan on the CPU, as the first for which every
one of the 64 permutations of all three cases keeps its top two tsq apart by more than 1e-7 relative, so none is left out; the
test asserts that count.  The hold-out seeds (101 to calibrate, 202 to hold out) are the function's default and its double, fixed
before anything was run."""
import math

import numpy as np
import pytest

from eagleeverything_amd import am, rcpp_api, synth
from test_gpu_repeated_measures import planted_case

pytestmark = pytest.mark.gpu
R = 64
SEED = {"geno_150x100": 3, "genoDemo_150x4998": 9}


def _geno(golden, name, tmp_path):
    g = golden(name)
    return g, synth.write_geno_pair(str(tmp_path), np.ascontiguousarray(g["M8"].T))


@pytest.mark.parametrize("cov,nan_rows", [(True, ()), (False, ()), (True, (3, 77, 149))])
@pytest.mark.parametrize("name", ["geno_150x100", "genoDemo_150x4998"])
def test_FPR4AM_is_the_AM_loop_on_permuted_traits(golden, tmp_path, monkeypatch, name, cov, nan_rows):
    g, geno = _geno(golden, name, tmp_path)
    y = g["y"].copy()
    y[list(nan_rows)] = np.nan
    X = g["X"] if cov else np.ones((y.size, 1))
    seed = SEED[name]
    res = am.FPR4AM(y, X, geno, falseposrate=0.1, numreps=R, seed=seed)
    np.testing.assert_array_equal(res["indxNA"], np.array(sorted(nan_rows, reverse=True), dtype=np.int64) + 1)
    keep = ~np.isnan(y)
    n, L, q = int(keep.sum()), g["M8"].shape[1], X.shape[1]
    c = am._lchoose(L, q) - am._lchoose(L, q - 1)
    np.testing.assert_array_equal(res["gamma_star"], (2.0 * (res["ML1"] - res["ML0"]) - math.log(n)) / (2.0 * c))
    assert res["setgamma"] == am.choose_gamma(res["gamma_star"], 0.1)
    assert res["falseposrate"] == am.fpr_curve(res["gamma_star"], res["setgamma"])[0] <= 0.1

    scans = []
    single = rcpp_api.spectral_scan

    def recording(*a, **kw):
        out = single(*a, **kw)
        scans.append(out)
        return out

    monkeypatch.setattr(rcpp_api, "spectral_scan", recording)
    rng = np.random.default_rng(seed)
    left_out = 0
    for r in range(R):
        yr = np.full(y.size, np.nan)
        yr[keep] = y[keep][rng.permutation(n)]
        del scans[:]
        ref = am.AM(yr, X, geno, maxit=2, backend=am.SpectralBackend())
        with np.errstate(all="ignore"):
            tsq = scans[0]["a"].ravel() ** 2 / scans[0]["vara"].ravel()
        top = np.sort(tsq[~np.isnan(tsq)])[::-1]
        tr = ref["extBIC_trace"]
        print("r=%d pick %d/%d top-two gap %.2e ML0 %.3e ML1 %.3e" % (
            r, res["picks"][r], ref["all_picks"][0], (top[0] - top[1]) / top[0],
            abs(-2 * res["ML0"][r] + (q + 1) * math.log(n) + 2 * am._lchoose(L, q - 1) - tr[0]) / abs(tr[0]),
            abs(-2 * res["ML1"][r] + (q + 2) * math.log(n) + 2 * am._lchoose(L, q) - tr[1]) / abs(tr[1])))
        np.testing.assert_allclose(-2 * res["ML0"][r] + (q + 1) * math.log(n) + 2 * am._lchoose(L, q - 1), tr[0], rtol=1e-8)
        if (top[0] - top[1]) < 1e-9 * top[0]:
            left_out += 1
            continue
        assert res["picks"][r] == ref["all_picks"][0], r
        assert res["tsqmax"][r] == pytest.approx(top[0], rel=1e-6)
        np.testing.assert_allclose(-2 * res["ML1"][r] + (q + 2) * math.log(n) + 2 * am._lchoose(L, q), tr[1], rtol=1e-8)
        assert (tr[1] < tr[0]) == (1 < res["gamma_star"][r]), r
    assert left_out == 0                                              # the committed seeds have no near tie (2 % would be allowed)
    rcpp_api.drop_cache()


def _equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_FPR4AM_seed_chunk_eig_and_two_contexts(golden, tmp_path, monkeypatch):
    g, geno = _geno(golden, "genoDemo_150x4998", tmp_path)
    y, X = g["y"], g["X"]
    prepares = []
    prepare = rcpp_api.spectral_prepare
    monkeypatch.setattr(rcpp_api, "spectral_prepare", lambda *a, **kw: (prepares.append(kw.get("device", 0)), prepare(*a, **kw))[1])
    a = am.FPR4AM(y, X, geno, numreps=R, seed=9)
    assert prepares == [0]
    _equal(a, am.FPR4AM(y, X, geno, numreps=R, seed=9))               # the same seed twice
    assert prepares == [0]                                            # ... on the Z still resident
    c5 = am.FPR4AM(y, X, geno, numreps=R, seed=9, chunk=5)
    np.testing.assert_array_equal(c5["gamma_star"], a["gamma_star"])
    np.testing.assert_array_equal(c5["picks"], a["picks"])
    assert c5["setgamma"] == a["setgamma"] and c5["falseposrate"] == a["falseposrate"]
    np.testing.assert_allclose(c5["tsqmax"], a["tsqmax"], rtol=1e-10)   # other column groups: the figure of test_gpu_traits.py
    assert not np.array_equal(am.FPR4AM(y, X, geno, numreps=R, seed=10)["gamma_star"], a["gamma_star"])
    # eig= from an AM() run on the SpectralBackend: no eigh, and no prepare either (AM left this Z resident)
    rcpp_api.drop_cache()
    be = am.SpectralBackend()
    am.AM(y, X, geno, maxit=2, backend=be)
    n0 = len(prepares)
    _equal(a, am.FPR4AM(y, X, geno, numreps=R, seed=9, eig=be.eig))
    assert len(prepares) == n0
    rcpp_api.drop_cache()
    # two sub-contexts on one card shard the markers of every scan
    two = am.FPR4AM(y, X, geno, numreps=R, seed=9, device=(0, 0))
    rcpp_api.drop_cache(device=(0, 0))
    np.testing.assert_array_equal(two["picks"], a["picks"])
    np.testing.assert_array_equal(two["gamma_star"], a["gamma_star"])
    assert two["setgamma"] == a["setgamma"]


def test_calibrated_gamma_holds_its_rate_on_fresh_permutations(golden, tmp_path):
    g, geno = _geno(golden, "genoDemo_150x4998", tmp_path)
    y, X = g["y"], g["X"]
    Rh, fpr = 400, 0.1
    cal = am.FPR4AM(y, X, geno, falseposrate=fpr, numreps=Rh, seed=101)
    assert cal["falseposrate"] <= fpr
    rng = np.random.default_rng(202)
    Y = np.column_stack([y[rng.permutation(y.size)] for _ in range(Rh)])
    out = am.AM_traits(Y, X, geno, maxit=2, gamma=cal["setgamma"])
    share = float(np.mean([o["extBIC_trace"][1] < o["extBIC_trace"][0] for o in out]))   # AM.R:448: the first pick is kept
    # the hold-out share is binomial(400, p): 3 sigma at p = 0.1; the calibration set fixes its own rate only to one step 1/400
    bound = 3.0 * math.sqrt(fpr * (1.0 - fpr) / Rh) + 1.0 / Rh
    print("setgamma %.6f, FPR on the calibration set %.4f, hold-out share %.4f, bound %.4f" % (cal["setgamma"], cal["falseposrate"], share, bound))
    assert abs(share - fpr) <= bound
    rcpp_api.drop_cache()


def test_calibrated_gamma_keeps_the_planted_loci(tmp_path):
    Mt8, M, ind, y, X, planted = planted_case(reps=1)                 # Z = I: one record per individual
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    be = am.SpectralBackend()
    one = am.AM(y, X, geno, maxit=12, backend=be)
    cal = am.FPR4AM(y, X, geno, falseposrate=0.05, numreps=200, seed=101, eig=be.eig)
    res = am.AM(y, X, geno, maxit=12, backend=am.SpectralBackend(), gamma=cal["setgamma"])
    print("setgamma %.6f: %s against %s at gamma = 1" % (cal["setgamma"], res["selected_loci"], one["selected_loci"]))
    assert set(p + 1 for p in planted) <= set(one["selected_loci"]) <= set(res["selected_loci"])
    rcpp_api.drop_cache()
