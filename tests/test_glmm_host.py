"""CPU: the logistic mixed model's host side (eagleeverything_amd/glmm.py) -- the numpy restatement of the saddlepoint rule of
include/eagle_hip.h section 1d''' against 40-digit roots (tests/glmm_truth.py), the rule itself against full enumeration of the 2^18
outcomes, every code on planted markers, the fixed point of null_fit by plain dense algebra, the tau = 0 model against Logistic's
score test, and what the kinship term is for: a structured panel.  No device work."""
import numpy as np
import pytest

import glmm_truth as truth

TOL = 1e-10


def host_panel(n, L, c, seed, cutoff):
    from eagleeverything_amd import glmm
    Mt8, mu, r, X, vs = truth.panel(n, L, c, seed)
    V = glmm.spa_host(Mt8, mu, r, X, cutoff=1e9)[0][:, 1] * vs                  # V*, scaled where the fixture says so
    stat, info = glmm.spa_host(Mt8, mu, r, X, vara=V, cutoff=cutoff, tol=TOL)
    return Mt8, mu, r, X, V, stat, info


def check_against_truth(name, Mt8, mu, r, X, V, stat, info, cutoff, rows=None):
    """Codes equal the 40-digit rule's, T, V* and z agree to their summation bounds, ln p lies within glmm_truth.allowance."""
    worst = 0.0
    for m in (range(Mt8.shape[0]) if rows is None else rows):
        t = dict(truth.truth(mu, X, Mt8[m] + 1.0, r, V=V[m]))                  # the rule without a screen, shared by both cutoffs
        if t["code"] != 2 and abs(t["z"]) <= cutoff:
            t["code"] = 4
        assert info[m, 0] == t["code"], (name, m, info[m], t["code"])
        assert abs(stat[m, 0] - t["T"]) <= 4 * len(mu) * 2.0 ** -53 * np.sum(np.abs((Mt8[m] + 1.0) * r)), (name, m)
        if t["code"] == 2:
            assert np.all(np.isnan(stat[m, 2:])) and info[m, 1] == 0
            continue
        assert abs(stat[m, 2] / t["z"] - 1.0) <= 1e-11, (name, m)
        if t["code"] in (3, 4):
            assert np.all(np.isnan(stat[m, 3:])) and info[m, 1] == (0 if t["code"] == 4 else 1)
            continue
        err, allow = abs(truth.lnp_of(stat[m]) - t["lnp"]), truth.allowance(t, TOL)
        worst = max(worst, err / allow)
        assert err <= allow, (name, m, err, allow)
        assert info[m, 1] >= 3
        if t["code"] == 256:
            assert np.isinf(stat[m, 4]) or np.isinf(stat[m, 6])
    print("%s: worst ln p error / allowance %.3g" % (name, worst))
    return worst


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("n,L,c", [(5, 5, 1), (63, 8, 4), (64, 5, 4), (65, 8, 15), (257, 5, 4), (65, 5, 1)])
@pytest.mark.parametrize("cutoff", [0.0, 2.0])
def test_spa_host_against_truth(n, L, c, cutoff):
    """spa_host's ln p within the stop rule's share |d ln p / d zeta| tol / sqrt(V*) plus the first-order rounding term of
    glmm_truth (its docstring derives both).  Measured: the worst error is 0.66 of the allowance (n = 257, c = 15, a common marker whose
    w = sqrt(2 (zeta q - K)) cancels), 0.02 and below on every rare marker."""
    Mt8, mu, r, X, V, stat, info = host_panel(n, L, c, 100 + n, cutoff)
    check_against_truth("host n%d L%d c%d cutoff %g" % (n, L, c, cutoff), Mt8, mu, r, X, V, stat, info, cutoff)
    if cutoff == 2.0:
        assert np.all((info[:, 0] == 4) == (np.abs(stat[:, 2]) <= 2.0))


# ------------------------------------------------------------------------------------------------ 2. the rule against enumeration
def test_rule_against_full_enumeration():
    """n = 18, prevalence 0.1, MAF 0.1, default_rng(seed) for seeds 0 .. 29 drawing x = standard_normal(n) and then g = binomial(2, maf,
    n); fixtures with fewer than 3 carriers or fewer than 4 non-carriers are skipped; y = every carrier plus the first two non-carriers;
    mu = expit(logit 0.1 + 0.3 x), X = [1, x], tau = 0.  In every kept fixture the saddlepoint p-value is nearer the exact two-sided
    tail P(|S| >= |q|), S = sum G~_i (Y_i - mu_i) over all 2^18 outcomes, than the normal one.

    The recipe's mu is the model's, not a fit, so X'(y - mu) is not 0 and sum g_i (y_i - mu_i) is not the observed value of S (it lies
    outside S's support in every kept fixture).  The rule is therefore given the score residual r' = r - D X A X'r, for which
    sum g_i r'_i = sum G~_i r_i exactly as at a fixed point of the null fit; nothing else of the rule is touched.  With it the figures
    are the recipe's own: 22 fixtures kept, |log10(p_spa / p_exact)| <= 0.55, the normal p-value off by 0.69 to 3.06."""
    from eagleeverything_amd import glmm
    n, kept, spa_err, norm_err = 18, 0, [], []
    bits = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.float64)
    for seed in range(30):
        rng = np.random.default_rng(seed)
        x = rng.standard_normal(n)
        g = rng.binomial(2, 0.1, n)
        car, non = np.flatnonzero(g > 0), np.flatnonzero(g == 0)
        if car.size < 3 or non.size < 4:
            continue
        kept += 1
        y = np.zeros(n)
        y[car] = 1.0
        y[non[:2]] = 1.0
        mu = 1.0 / (1.0 + np.exp(-(np.log(0.1 / 0.9) + 0.3 * x)))
        X = np.column_stack([np.ones(n), x])
        D = mu * (1.0 - mu)
        A = np.linalg.inv(X.T @ (D[:, None] * X))
        gt = g - X @ (A @ (X.T @ (D * g)))
        r = y - mu
        stat, info = glmm.spa_host((g - 1).astype(np.int8)[None, :], mu, r - D * (X @ (A @ (X.T @ r))), X, A, cutoff=0.0, tol=TOL)
        pv = glmm.spa_pvalues(stat, info)
        assert info[0, 0] & 255 == 0, (seed, info)
        assert abs(stat[0, 0] - gt @ r) <= 1e-13
        q = stat[0, 2] * np.sqrt(stat[0, 1])
        S = (bits - mu[None, :]) @ gt
        logp = bits @ np.log(mu) + (1.0 - bits) @ np.log1p(-mu)
        slack = 1e-9 * np.sum(np.abs(gt))                                      # an outcome AT |q| (the observed one) belongs to the tail
        p_exact = float(np.sum(np.exp(logp[np.abs(S) >= abs(q) - slack])))
        e_spa, e_norm = abs(np.log10(pv["p_spa"][0] / p_exact)), abs(np.log10(pv["p_norm"][0] / p_exact))
        print("seed %d: p_exact %.3g spa %.3g normal %.3g" % (seed, p_exact, pv["p_spa"][0], pv["p_norm"][0]))
        assert e_spa < e_norm, (seed, e_spa, e_norm)
        spa_err.append(e_spa)
        norm_err.append(e_norm)
    assert kept >= 20, kept
    assert kept == 22 and max(spa_err) <= 0.555 and 0.685 <= min(norm_err) and max(norm_err) <= 3.065
    print("kept %d; |log10(p_spa / p_exact)| <= %.2f; normal %.2f .. %.2f" % (kept, max(spa_err), min(norm_err), max(norm_err)))


# ------------------------------------------------------------------------------------------------ 3. every code
def test_every_code_on_planted_markers():
    from eagleeverything_amd import glmm
    # 2 from a monomorphic marker, 3 from carriers = cases beyond the support, 4 below the cutoff, + 256 from five carriers of low mu with
    # four cases among them (c = 4), 0 elsewhere
    Mt8, mu, r, X, V, stat, info = host_panel(64, 8, 4, 164, 2.0)
    L = 8
    assert info[L - 1, 0] == 2 and info[L - 2, 0] == 256 and info[L - 3, 0] in (0, 4) and info[L - 4, 0] == 3
    assert abs(stat[L - 2, 2]) > 6 and stat[L - 2, 6] == -np.inf and np.isfinite(stat[L - 2, 4]) and stat[L - 2, 5] < 0
    assert (info[:, 0] == 4).any() and (info[:, 0] == 0).any()
    pv = glmm.spa_pvalues(stat, info)
    assert np.array_equal(pv["spa_used"], info[:, 0] & 255 == 0)
    assert np.array_equal(pv["p"][~pv["spa_used"]], pv["p_norm"][~pv["spa_used"]], equal_nan=True) and np.isnan(pv["p"][L - 1])
    assert np.array_equal(pv["p"][pv["spa_used"]], pv["p_spa"][pv["spa_used"]]) and pv["p_spa"][L - 2] > pv["p_norm"][L - 2]   # the normal tail is far too small
    # 3 at the edge of the support itself: intercept only, mu the fit, the carriers are the cases, V = V*
    n = 40
    y = np.zeros(n)
    y[[3, 17, 30]] = 1.0
    mu1 = np.full(n, y.mean())
    s1, i1 = glmm.spa_host((y - 1).astype(np.int8)[None, :], mu1, y - mu1, np.ones((n, 1)), cutoff=0.0)
    assert i1[0, 0] == 3 and i1[0, 1] == 1 and np.isfinite(s1[0, :3]).all() and np.isnan(s1[0, 3:]).all()
    # 2 from a marker equal to a column of X, and from a V that is not positive or not finite
    gx = np.random.default_rng(3).binomial(2, 0.3, 64).astype(np.float64)
    X2 = np.column_stack([np.ones(64), gx])
    s2, i2 = glmm.spa_host((gx - 1).astype(np.int8)[None, :], mu, r, X2, cutoff=0.0)
    assert i2[0, 0] == 2 and i2[0, 1] == 0
    for bad in (0.0, -1.0, np.inf, np.nan):
        Vb = V.copy()
        Vb[0] = bad
        assert glmm.spa_host(Mt8, mu, r, X, vara=Vb, cutoff=0.0)[1][0, 0] == 2
    # 1 from max_iter = 1: the reachability evaluation uses it up
    s3, i3 = glmm.spa_host(Mt8, mu, r, X, vara=V, cutoff=0.0, max_iter=1)
    solved = (info[:, 0] & 255 == 0) | (info[:, 0] == 4)
    assert np.all(i3[solved, 0] == 1) and np.all(i3[solved, 1] == 1) and np.all(np.isnan(s3[solved, 3:]))
    assert i3[L - 1, 0] == 2 and i3[L - 4, 0] == 3


# ------------------------------------------------------------------------------------------------ 4. the null model
def relatives(n, seed, L=400):
    """y, X, K of a panel of sib-like pairs with a random effect on K."""
    rng = np.random.default_rng(seed)
    G = rng.binomial(2, 0.3, size=(n, L)).astype(np.float64)
    for i in range(0, n - 1, 2):
        mix = rng.random(L) < 0.6
        G[i + 1, mix] = G[i, mix]
    Z = (G - G.mean(0)) / G.std(0)
    K = Z @ Z.T / L
    X = np.column_stack([np.ones(n), rng.standard_normal(n)])
    b = np.linalg.cholesky(K + 1e-8 * np.eye(n)) @ rng.standard_normal(n) * np.sqrt(1.2)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(-0.5 + 0.5 * X[:, 1] + b)))).astype(np.float64)
    return y, X, K


def dense(fit, y, X, K):
    """The fixed point's quantities by plain dense algebra at the fit's eta and tau."""
    tau, D, Y = fit["tau"], fit["D"], fit["Y"]
    Si = np.linalg.inv(np.diag(1.0 / D) + tau * K)
    C = np.linalg.inv(X.T @ Si @ X)
    alpha = C @ (X.T @ (Si @ Y))
    P = Si - Si @ X @ C @ X.T @ Si
    return alpha, tau * K @ (Si @ (Y - X @ alpha)), 0.5 * Y @ P @ K @ P @ Y - 0.5 * np.trace(P @ K), P


@pytest.mark.parametrize("n,seed", [(60, 1), (150, 2)])
def test_null_fit_fixed_point(n, seed):
    """alpha is the GLS estimate, b = tau K Sigma^-1 (Y - X alpha), and 1/2 Y'PKPY - 1/2 tr(PK) = 0 at an interior tau.  Tolerances: the
    fit stops when eta moves by <= tol, so the (alpha, b) returned solve the equations of an eta within tol of the one returned; the
    working vector Y = eta + (y - mu) / D moves by at most (1 + 1 / min D + |y - mu| |1 - 2 mu| / min D) tol <= 3 tol / min D^2, and
    alpha, b are linear in Y with operators of norm <= cond(Sigma) -- allowed: 3 cond(Sigma) tol / min D^2.  The score is quadratic in Y:
    relative to its two halves, 1/2 tr(PK), the same allowance twice, plus the tau search's own xtol of 1e-13 in ln tau."""
    from eagleeverything_amd import glmm
    tol = 1e-10
    y, X, K = relatives(n, seed)
    fit = glmm.null_fit(y, X, K, tol=tol)
    assert fit["converged"] and 2 <= fit["iterations"] <= 100 and glmm.TAU_MIN < fit["tau"] < glmm.TAU_MAX
    alpha, b, score, P = dense(fit, y, X, K)
    cond = np.linalg.cond(np.diag(1.0 / fit["D"]) + fit["tau"] * K)
    allow = 3.0 * cond * tol / fit["D"].min() ** 2
    print("n %d: tau %.4f, %d iterations, alpha %.2e b %.2e score %.2e of tr %.2f (allowed %.2e)"
          % (n, fit["tau"], fit["iterations"], np.abs(alpha - fit["alpha"]).max(), np.abs(b - fit["b"]).max(), score, 0.5 * np.trace(P @ K), allow))
    assert np.abs(alpha - fit["alpha"]).max() <= allow and np.abs(b - fit["b"]).max() <= allow
    assert abs(score) <= (2.0 * allow + 1e-11) * 0.5 * np.trace(P @ K)
    # what the scan takes: P and P Y = y - mu, and X'(y - mu) = 0
    assert np.abs(P - fit["P"]).max() <= 1e-12 * np.abs(P).max() * cond
    assert np.abs(fit["PY"] - (y - fit["mu"])).max() <= allow and np.abs(X.T @ (y - fit["mu"])).max() <= allow * n
    assert np.allclose(fit["eta"], X @ fit["alpha"] + fit["b"], rtol=0, atol=1e-12) and np.array_equal(fit["D"], fit["mu"] * (1 - fit["mu"]))


def test_null_fit_at_tau_zero():
    from eagleeverything_amd import glmm, r_api
    n = 60
    rng = np.random.default_rng(1)
    X = np.column_stack([np.ones(n), rng.standard_normal(n)])
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(-0.3 + 0.5 * X[:, 1])))).astype(np.float64)
    fit = glmm.null_fit(y, X, np.eye(n), tol=1e-10)                              # K = I and no structure: nothing for tau to explain
    assert fit["tau"] == 0.0 and fit["converged"]
    _, _, score, _ = dense(fit, y, X, np.eye(n))
    assert score <= 0.0                                                          # the boundary inequality
    assert np.all(fit["b"] == 0.0)
    a0 = r_api.logistic_null_host(X, y)
    assert np.abs(fit["alpha"] - a0).max() <= 1e-9
    # tau = 0.0 given: logistic_null_host's alpha, whatever K is
    y2, X2, K2 = relatives(60, 1)
    f0 = glmm.null_fit(y2, X2, K2, tau=0.0)
    assert f0["tau"] == 0.0 and f0["converged"] and np.abs(f0["alpha"] - r_api.logistic_null_host(X2, y2)).max() <= 1e-12
    for bad in (dict(tau=-1.0), dict(tau=1e-6), dict(tau=1e5), dict(tol=0.0), dict(max_iter=0)):
        with pytest.raises(ValueError):
            glmm.null_fit(y2, X2, K2, **bad)
    with pytest.raises(ValueError):
        glmm.null_fit(np.ones(60), X2, K2)
    with pytest.raises(ValueError):
        glmm.null_fit(y2, X2, K2[:59, :59])


def test_tau_zero_score_is_logistic_hosts():
    """With tau = 0 the model is Logistic's and T^2 / V its score test: V* = sum D G~^2 is the Schur complement 1 / (I^-1)_gg that
    logistic_host takes from its Cholesky factor.  Two fp64 evaluations of the same sums in two orders: T carries n 2^-53 sum |g r| / |T|
    each, V the magnitudes of its two halves sum D g^2 + sum D (x'beta)^2 over V*, the factor's half times cond(X'DX) for the columns
    before the marker's; a factor 4 for the products inside the terms."""
    from eagleeverything_amd import glmm, r_api
    rng = np.random.default_rng(9)
    n, L, c = 150, 40, 3
    X = truth.covariates(n, c, 10)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(-1.0 + 0.6 * X[:, 1])))).astype(np.float64)
    Mt8 = (rng.binomial(2, 0.2, size=(L, n)) - 1).astype(np.int8)
    fit = glmm.null_fit(y, X, np.eye(n), tau=0.0, tol=1e-12)
    stat, info = glmm.spa_host(Mt8, fit["mu"], y - fit["mu"], X, fit["A"], cutoff=0.0)
    want = r_api.logistic_host(Mt8, y.astype(np.int64), X, firth=0, tol=1e-12, max_iter=1, beta0=fit["alpha"])[0][:, 2]
    D, eps = fit["D"], 2.0 ** -53
    condX = np.linalg.cond(X.T @ (D[:, None] * X))
    for m in range(L):
        g = Mt8[m] + 1.0
        xb = X @ (fit["A"] @ (X.T @ (D * g)))
        relT = n * eps * np.sum(np.abs(g * (y - fit["mu"]))) / abs(stat[m, 0])
        relV = n * eps * (np.sum(D * g * g) + condX * np.sum(D * xb * xb)) / stat[m, 1]
        got = stat[m, 2] ** 2
        assert abs(got - want[m]) <= 4.0 * (2.0 * 2.0 * relT + 2.0 * relV) * want[m], (m, got, want[m])


# ------------------------------------------------------------------------------------------------ 5. what the kinship term is for
def test_structured_panel_is_less_inflated_than_logistic():
    """Two sub-populations of 100 with drifted allele frequencies and prevalences 0.15 and 0.5, no causal marker, 400 markers,
    restatements only.  Intercept-only Logistic has nothing that knows the structure and its median score is 3.99 times the chi^2_1
    median; GLMM with K = MM'/max + 0.95 I, as calcMMt makes it, is at 1.33 (tau = 0.58)."""
    from scipy.special import chdtri
    from eagleeverything_amd import glmm, r_api
    n, L = 200, 400
    rng = np.random.default_rng(0)
    p0 = rng.uniform(0.1, 0.5, L)
    pa, pb = np.clip(p0 + 0.15 * rng.standard_normal(L), 0.03, 0.97), np.clip(p0 - 0.15 * rng.standard_normal(L), 0.03, 0.97)
    G = np.vstack([rng.binomial(2, pa, size=(n // 2, L)), rng.binomial(2, pb, size=(n // 2, L))])
    y = np.concatenate([rng.random(n // 2) < 0.15, rng.random(n // 2) < 0.5]).astype(np.float64)
    Mt8 = (G.T - 1).astype(np.int8)
    M = Mt8.T.astype(np.float64)
    K = M @ M.T
    K = K / K.max() + 0.95 * np.eye(n)
    X = np.ones((n, 1))
    fit = glmm.null_fit(y, X, K)
    assert fit["converged"] and fit["tau"] > 0.1
    V = np.einsum("li,ij,lj->l", M.T, fit["P"], M.T)
    stat, info = glmm.spa_host(Mt8, fit["mu"], y - fit["mu"], X, fit["A"], V)
    cols = glmm.glmm_columns(stat, info, V)
    logistic = r_api.logistic_host(Mt8, y.astype(np.int64), X, firth=0, max_iter=1, beta0=r_api.logistic_null_host(X, y))[0][:, 2]
    med = chdtri(1.0, 0.5)
    lam_glmm, lam_logistic = np.nanmedian(cols["score"]) / med, np.nanmedian(logistic) / med
    print("lambda: GLMM %.3f, Logistic %.3f (tau %.3f)" % (lam_glmm, lam_logistic, fit["tau"]))
    assert abs(lam_glmm - 1.0) < abs(lam_logistic - 1.0) and lam_logistic > 2.0 and lam_glmm < 2.0
    assert np.allclose(cols["beta"], stat[:, 0] / V) and np.allclose(cols["se"], 1 / np.sqrt(V)) and np.allclose(cols["score"], stat[:, 0] ** 2 / V)
