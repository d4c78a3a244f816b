"""CPU: r_api.logistic_host, the numpy restatement of include/eagle_hip.h section 1b''''iv, held to what does not come from it -- the
40-digit roots of tests/logistic_truth.py, the closed forms of a saturated 2 x 2 table (Woolf; Firth = half added to every cell), the
Cochran-Armitage trend statistic of case_control_from_counts for the score test -- and the codes of monomorphic and separated
markers.  Also: entries of tests/golden/logistic_truth.npz recomputed live.  No device work."""
import math

import numpy as np
import pytest

import logistic_truth as truth

TOL = 1e-10


def small_panel(n, c, seed, L=4):
    from eagleeverything_amd import synth
    X = truth.covariates(n, c, seed)
    st = truth.draw_status(X, seed + 1)
    Mt8 = synth.genotypes_marker_major(n, 64, seed=seed + 2)
    maf_ok = np.minimum((Mt8 + 1).sum(axis=1), (1 - Mt8).sum(axis=1)) >= n // 2       # no rare markers at these sizes
    return np.ascontiguousarray(Mt8[maf_ok][:L]), st, X


def check_against_truth(Mt8, st, X, firth_rows=()):
    """Every marker: where the truth's ML fit exists with a clear margin the restatement converges to it within the bounds of
    logistic_truth.ml_bounds; where it does not exist the restatement says so.  Firth likewise for firth_rows."""
    from eagleeverything_amd import r_api
    n = X.shape[0]
    stat, info = r_api.logistic_host(Mt8, st, X, 0, TOL, 50)
    statf, infof = r_api.logistic_host(Mt8, st, X, 1, TOL, 200)
    seen = 0
    for m in range(Mt8.shape[0]):
        t = truth.marker_truth(Mt8[m].astype(np.int64) + 1, st, X, firth=m in firth_rows)
        if t["ok"] and t["maxeta"] <= truth.ETA_CLEAR and t["cond"] <= 1e6:
            bg, rse, rll = truth.ml_bounds(n, TOL, t)
            print("n %d c %d marker %d: gamma err %.3g (bound %.3g), se rel %.3g (%.3g), ll rel %.3g (%.3g)" % (
                n, X.shape[1], m, abs(stat[m, 0] - t["gamma"]), bg, abs(stat[m, 1] / t["se"] - 1), rse, abs(stat[m, 3] / t["ll"] - 1), rll))
            assert info[m, 0] == 0
            assert abs(stat[m, 0] - t["gamma"]) <= bg
            assert abs(stat[m, 1] - t["se"]) <= rse * t["se"]
            assert abs(stat[m, 3] - t["ll"]) <= rll * abs(t["ll"])
            seen += 1
        elif not t["ok"]:
            assert info[m, 0] != 0 and np.isnan(stat[m, 0]) and np.isnan(stat[m, 1])
        if m in firth_rows and t["f_ok"] and t["f_cond"] <= 1e6:
            assert t["f_ratio"] <= 0.9
            bg, rse = truth.firth_bounds(n, TOL, t)
            assert infof[m, 0] == 256
            assert abs(statf[m, 0] - t["f_gamma"]) <= bg
            assert abs(statf[m, 1] - t["f_se"]) <= rse * t["f_se"]
    return seen


@pytest.mark.parametrize("n,c", [(40, 1), (40, 3), (40, 15), (203, 1), (203, 3), (203, 15)])
def test_host_against_the_40_digit_roots(n, c):
    Mt8, st, X = small_panel(n, c, 10 * n + c, L=3 if c == 15 else 4)
    seen = check_against_truth(Mt8, st, X, firth_rows=() if c == 15 else (0,))
    assert seen >= (0 if (n, c) == (40, 15) else 2)                  # 16 parameters on 36 individuals: a fit need not exist


def table_panel(a, b, c, d, copies=2):
    """carriers (g = copies): a cases, b controls; the others (g = 0): c cases, d controls; intercept only."""
    g = np.array([copies] * (a + b) + [0] * (c + d))
    y = np.array([1] * a + [0] * b + [1] * c + [0] * d, dtype=np.int32)
    return (g - 1).astype(np.int8)[None, :], y, np.ones((g.size, 1))


@pytest.mark.parametrize("cells", [(7, 4, 5, 9), (30, 11, 17, 40), (3, 12, 20, 6)])
def test_saturated_table_closed_forms(cells):
    from eagleeverything_amd import r_api
    a, b, c, d = cells
    Mt8, y, X = table_panel(a, b, c, d)
    stat, info = r_api.logistic_host(Mt8, y, X, 0, TOL, 50)
    assert info[0, 0] == 0
    assert abs(stat[0, 0] - 0.5 * math.log(a * d / (b * c))) <= 1e-9                      # per allele copy: g is 0 or 2
    assert abs(stat[0, 1] - 0.5 * math.sqrt(1 / a + 1 / b + 1 / c + 1 / d)) <= 1e-9      # Woolf, halved
    statf, infof = r_api.logistic_host(Mt8, y, X, 1, TOL, 100)
    assert infof[0, 0] == 256
    assert abs(statf[0, 0] - 0.5 * math.log((a + .5) * (d + .5) / ((b + .5) * (c + .5)))) <= 1e-8
    stat2, info2 = r_api.logistic_host(Mt8, y, X, 2, TOL, 50)                            # nothing to fall back from
    assert np.array_equal(info2, info) and np.array_equal(stat2, stat)


@pytest.mark.parametrize("cells", [(7, 0, 5, 9), (6, 8, 0, 11), (12, 0, 0, 9)])
def test_zero_cell_separates_and_falls_back(cells):
    from eagleeverything_amd import r_api
    a, b, c, d = cells
    Mt8, y, X = table_panel(a, b, c, d)
    stat, info = r_api.logistic_host(Mt8, y, X, 0, TOL, 50)
    # A zero cell among the carriers sends gamma away and ends in code 3 (or 1).  A zero cell among the NON-carriers sends the intercept
    # away: every weight outside the carriers vanishes, gamma's column becomes the intercept's to the resolution of fp64 near |eta| = 28,
    # and the fit ends in code 2 AFTER its first evaluation, which the fallback restarts all the same.
    assert info[0, 0] in ((1, 3) if b == 0 else (1, 2, 3)) and info[0, 1] > 1
    assert np.isnan(stat[0, 0]) and np.isnan(stat[0, 1]) and np.isfinite(stat[0, 2])
    stat2, info2 = r_api.logistic_host(Mt8, y, X, 2, TOL, 50)
    want = 0.5 * math.log((a + .5) * (d + .5) / ((b + .5) * (c + .5)))
    print("Firth %.12g against the closed form %.12g in %d evaluations" % (stat2[0, 0], want, info2[0, 1]))
    assert info2[0, 0] == 256 and abs(stat2[0, 0] - want) <= 1e-8
    assert stat2[0, 2] == stat[0, 2]                                                     # the score is the first evaluation's


def test_score_is_the_trend_test_at_c_1():
    from eagleeverything_amd import r_api, synth
    n, L = 203, 80
    Mt8 = synth.genotypes_marker_major(n, L, seed=5)
    st = truth.draw_status(np.ones((n, 1)), 6)
    stat, _ = r_api.logistic_host(Mt8, st, np.ones((n, 1)), 0, TOL, 50)
    trend = r_api.case_control_from_counts(r_api.group_counts_host(Mt8, st, 2))["trend"]
    ok = np.isfinite(trend)
    assert ok.sum() >= L - 2
    assert np.all(np.abs(stat[ok, 2] - trend[ok]) <= 1e-12 * trend[ok])


def test_monomorphic_rows_give_code_2():
    from eagleeverything_amd import r_api
    n = 67
    for c in (1, 4):
        X = truth.covariates(n, c, 77 + c)
        st = truth.draw_status(X, 78 + c)
        Mt8 = np.stack([np.full(n, v, dtype=np.int8) for v in (-1, 0, 1)])
        mono_among_used = np.where(st >= 0, 1, np.arange(n) % 3 - 1).astype(np.int8)     # varies only among the unused individuals
        Mt8 = np.vstack([Mt8, mono_among_used[None, :]])
        for firth in (0, 1, 2):
            stat, info = r_api.logistic_host(Mt8, st, X, firth, TOL, 50)
            assert np.array_equal(info[:, 0], np.full(4, 2 + (256 if firth == 1 else 0))) and np.array_equal(info[:, 1], np.ones(4))
            assert np.all(np.isnan(stat))


def test_null_fit_and_interface_checks():
    from eagleeverything_amd import r_api
    X = truth.covariates(100, 3, 1)
    y = truth.draw_status(X, 2)
    used = y >= 0
    b0 = r_api.logistic_null_host(X[used], y[used])
    mu = 1 / (1 + np.exp(-X[used] @ b0))
    assert np.max(np.abs(X[used].T @ (y[used] - mu))) <= 1e-9                             # the score equations hold
    with pytest.raises(ValueError):
        r_api.logistic_null_host(np.column_stack([X[used], X[used][:, 1]]), y[used])     # collinear
    with pytest.raises(ValueError):
        r_api.logistic_null_host(X[used], (X[used][:, 1] > 0).astype(int))               # separated by a covariate


def test_golden_truth_is_what_the_helper_computes():
    """Entries of the stored truth, recomputed: the file is the helper's output for today's panels."""
    for name, rows in (("c1", (0, 96)), ("n67", (3,)), ("L5", (2,)), ("n20", (11,))):
        Mt8, st, X, fr, t = truth.golden(name)
        for m in rows:
            live = truth.marker_truth(Mt8[m].astype(np.int64) + 1, st, X, firth=m in fr)
            for k in truth.FIELDS + truth.FIRTH_FIELDS:
                assert (np.isnan(live[k]) and np.isnan(t[k][m])) or abs(live[k] - t[k][m]) <= 1e-13 * abs(live[k]), (name, m, k)
    for name in truth.all_panels():                                                      # the coverage the GPU tests rely on
        Mt8, st, X, fr, t = truth.golden(name)
        good = (t["ok"] == 1) & (t["maxeta"] <= truth.ETA_CLEAR) & (t["cond"] <= 1e6)
        assert good.mean() > 0.95 or Mt8.shape[0] < 8, (name, good.mean())
