"""CPU: the admixture rule of include/eagle_hip.h section 1b''''v as r_api.admixture_host restates it, and the driver r_api.Admixture
on top of it (step=host), with no device.

  * one step and l against 40-digit arithmetic (tests/admixture_truth.py) within the derived bounds;
  * K = 1 gives clamp(mean(d) / 2); the rows of Q' sum to 1; permuting the individuals permutes the rows of Q';
  * on the planted panels l never falls over 300 steps;
  * the SQUAREM driver's trace never falls, reaches plain EM's 300-step l in fewer EM evaluations and recovers the planted Q."""
import numpy as np
import pytest

import admixture_truth as truth

_cache = {}


def em300(n, L, K):
    """(Mt8, planted Q, start Q0, F0, the 300-step host result), computed once per panel."""
    from eagleeverything_amd import r_api
    key = (n, L, K)
    if key not in _cache:
        Mt8, Qt, _ = truth.planted_panel(n, L, K, 1)
        Q0, F0 = r_api.admixture_init(n, L, K, 1, truth.marker_freq(Mt8))
        _cache[key] = (Mt8, Qt, Q0, F0, r_api.admixture_host(Mt8, Q0, F0, 300))
    return _cache[key]


def host_step(Mt8):
    from eagleeverything_amd import r_api
    return lambda f, dims, Q, F, steps=1: r_api.admixture_host(Mt8, Q, F, steps)


def geno_of(Mt8):
    return {"asciifileM": "unused", "asciifileMt": "unused", "dim_of_ascii_M": [Mt8.shape[1], Mt8.shape[0]]}


@pytest.mark.parametrize("K", truth.HOST_KS)
@pytest.mark.parametrize("n,L", truth.HOST_SHAPES)
def test_one_step_against_mpmath(n, L, K):
    from eagleeverything_amd import r_api
    Mt8, _, _ = truth.planted_panel(n, L, max(K, 2), 10 * n + K)
    Q, F = truth.planted_inputs(n, L, K, n + L + K)
    Qn, Fn, ll = r_api.admixture_host(Mt8, Q, F, 1)
    wQ, wF, wl = truth.mp_step(Mt8, Q, F)
    assert ll.shape == (2,)
    truth.assert_close((Qn, Fn, ll[0]), (wQ, wF, wl), n, L, K, "host")
    _, _, wl1 = truth.mp_step(Mt8, Qn, Fn)                          # the second entry is l at the returned parameters
    assert abs(ll[1] - wl1) <= truth.ll_bound(n, L, K, wl1)
    Q0, F0, l0 = r_api.admixture_host(Mt8, Q, F, 0)                 # steps = 0: the likelihood alone
    assert np.array_equal(Q0, Q) and np.array_equal(F0, F) and l0.shape == (1,) and l0[0] == ll[0]


@pytest.mark.parametrize("n,L", truth.HOST_SHAPES + [(120, 600)])
def test_K1_one_step_gives_the_mean_dosage(n, L):
    from eagleeverything_amd import r_api
    Mt8, _, _ = truth.planted_panel(n, L, 2, n)
    Q, F = truth.planted_inputs(n, L, 1, 5)
    assert np.array_equal(Q, np.ones((n, 1)))
    Qn, Fn, _ = r_api.admixture_host(Mt8, Q, F, 1)
    want = np.clip(truth.marker_freq(Mt8), truth.EPS, 1.0 - truth.EPS)
    assert np.array_equal(Qn, Q)
    assert np.max(np.abs(Fn[:, 0] - want) / want) <= truth.rel_bound(n, L, 1)
    assert Fn[0, 0] == truth.EPS and Fn[1, 0] == 1.0 - truth.EPS   # the all-0 and the all-2 marker meet the clamps


@pytest.mark.parametrize("n,L,K", truth.EM_PANELS)
def test_rows_of_Q_sum_to_one_and_loglik_never_falls(n, L, K):
    Mt8, _, _, _, (Q, F, ll) = em300(n, L, K)
    assert np.max(np.abs(Q.sum(axis=1) - 1.0)) <= 4 * 2.0 ** -52
    assert Q.min() > 0.0 and F.min() >= truth.EPS and F.max() <= 1.0 - truth.EPS
    d = np.diff(ll)
    print("n=%d L=%d K=%d: l %.17g -> %.17g, smallest increase %.3g (%.3g of |l|)" % (n, L, K, ll[0], ll[-1], d.min(), d.min() / abs(ll[-1])))
    assert ll.shape == (301,) and np.all(np.isfinite(ll))
    assert np.all(d >= 0.0)


def test_permuting_the_individuals_permutes_the_rows():
    from eagleeverything_amd import r_api
    n, L, K = 33, 50, 5
    Mt8, _, _ = truth.planted_panel(n, L, K, 3)
    Q, F = truth.planted_inputs(n, L, K, 4)
    perm = np.random.default_rng(5).permutation(n)
    Qa, Fa, la = r_api.admixture_host(Mt8, Q, F, 1)
    Qb, Fb, lb = r_api.admixture_host(np.ascontiguousarray(Mt8[:, perm]), Q[perm], F, 1)
    truth.assert_close((Qb, Fb, lb[0], lb[1]), (Qa[perm], Fa, la[0], la[1]), n, L, K, "permuted")


def test_driver_on_the_host_step_squarem_against_plain_em():
    """The counts this prints are the ones DESIGN 4.8r records."""
    from eagleeverything_amd import r_api
    n, L, K = 120, 600, 3
    Mt8, Qt, Q0, F0, (_, _, ll300) = em300(n, L, K)
    r = r_api.Admixture(geno_of(Mt8), K, init=(Q0, F0), step=host_step(Mt8))
    tr = r["loglik"]
    assert r["converged"] and r["iterations"] == len(tr) - 1 and r["K"] == K
    assert np.all(np.diff(tr) >= 0.0)                                # the trace never falls
    assert tr[0] == ll300[0]
    reached = np.nonzero(tr >= ll300[-1])[0]
    print("plain EM: 300 evaluations to l = %.10g; SQUAREM reaches it after %s of its %d evaluations" % (ll300[-1], reached[:1], r["iterations"]))
    assert reached.size and reached[0] < 300
    plain = r_api.Admixture(geno_of(Mt8), K, init=(Q0, F0), step=host_step(Mt8), accel="none", max_iter=300, tol=1e-12)
    assert plain["iterations"] == 300 and abs(plain["loglik"][-1] - ll300[-1]) <= truth.ll_bound(n, L, K, ll300[-1])
    # the result: components by decreasing mean, Q rows on the simplex, F (K, L), the assignment
    assert r["Q"].shape == (n, K) and r["F"].shape == (K, L) and np.all(np.diff(r["Q"].mean(axis=0)) <= 0.0)
    assert np.max(np.abs(r["Q"].sum(axis=1) - 1.0)) <= 4 * 2.0 ** -52
    assert np.array_equal(r["assignment"], np.argmax(r["Q"], axis=1))
    corr = truth.best_permutation_corr(r["Q"], Qt)
    print("recovery: mean column correlation %.4f" % corr)
    assert corr >= 0.98
    # relabelling the start relabels nothing for the caller
    r2 = r_api.Admixture(geno_of(Mt8), K, init=(Q0[:, ::-1], F0[:, ::-1]), step=host_step(Mt8))
    assert np.allclose(r2["Q"], r["Q"], atol=1e-6) and np.array_equal(r2["assignment"], r["assignment"])


def test_add_ancestry_appends_all_but_the_last_column():
    from eagleeverything_amd import am
    Q = np.random.default_rng(0).dirichlet(np.ones(4), size=9)
    X = am.add_ancestry(np.ones(9), {"Q": Q})
    assert X.shape == (9, 4) and np.array_equal(X[:, 0], np.ones(9)) and np.array_equal(X[:, 1:], Q[:, :3])
    assert am.add_ancestry(np.ones((9, 2)), {"Q": Q[:, :1]}).shape == (9, 2)     # K = 1 adds nothing
    with pytest.raises(ValueError):
        am.add_ancestry(np.ones(8), {"Q": Q})


def test_init_is_seeded_and_admissible():
    from eagleeverything_amd import r_api
    Q, F = r_api.admixture_init(33, 50, 5, 7, np.linspace(0.0, 1.0, 50))
    Q2, F2 = r_api.admixture_init(33, 50, 5, 7, np.linspace(0.0, 1.0, 50))
    assert np.array_equal(Q, Q2) and np.array_equal(F, F2)
    assert Q.shape == (33, 5) and F.shape == (50, 5) and F.min() >= 0.05 and F.max() <= 0.95
    assert np.max(np.abs(Q.sum(axis=1) - 1.0)) <= 4 * 2.0 ** -52 and Q.min() > 0.0
    assert not np.array_equal(r_api.admixture_init(33, 50, 5, 8)[0], Q)
    with pytest.raises(ValueError):
        r_api.admixture_init(33, 50, 5, 7, np.ones(49))
