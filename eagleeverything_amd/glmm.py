"""Case/control association under the logistic mixed model: GMMAT's score test (Chen et al. 2016) with SAIGE's saddlepoint
approximation (SPA; Dey et al. 2017, Zhou et al. 2018) for the p-values.  No counterpart in the reference, whose trait is quantitative.

    null_fit(y, X, K)   the null model  logit mu = X alpha + b, b ~ N(0, tau K)  by penalised quasi-likelihood, on the host
                        (host_model.algebra() does the n^3 work, so the opt-in device algebra applies);
    spa(...)            eagle_glmm_spa: per marker the score T, its variance V*, and the saddlepoint deviates of both tails, on the
                        device (k_glmm_spa, csrc/eagle_glmm.hip; the rule is include/eagle_hip.h section 1d''');
    spa_host(...)       that rule restated in numpy, marker by marker;
    spa_pvalues(...)    the p-values of either's result;
    GLMM(geno, status)  the whole analysis; r_api.GLMM forwards here.

Agreement with the GMMAT, SAIGE or SPAtest programs is not claimed: none is at hand.  tests/glmm_truth.py holds spa and spa_host to
40-digit roots of the same equations, tests/test_glmm_host.py the rule itself to full enumeration at n = 18.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _lib, host_model

SPA_MAX_COVARIATES = 15
SPA_DEGENERATE, SPA_ZETA_RANGE, SPA_NEAR_ZERO = 2.0 ** -40, 500.0, 1e-4
TAU_MIN, TAU_MAX = math.exp(-10.0), math.exp(10.0)


# ---------------------------------------------------------------------------------------------------------------------------
# The per-marker rule: the device call and its numpy restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _spa_inputs(who, n, nm, mu, resid, X, A, vara, cutoff, tol, max_iter):
    """(mu, resid fp64 (n), X fp64 (n, c) column-major, A fp64 (c, c) column-major, vara fp64 (L) or None) after the checks
    eagle_glmm_spa makes, as ValueError.  A = None: (X'DX)^-1 is formed here."""
    def vec(a, name):
        v = np.asarray(a)
        if v.dtype.kind not in "iuf" or v.ndim != 1 or v.size != n:
            raise ValueError("%s: %s must hold one number per individual (%d)" % (who, name, n))
        return np.ascontiguousarray(v, dtype=np.float64)

    if n <= 0 or nm <= 0:
        raise ValueError("%s: dims must be positive" % who)
    muv, rv = vec(mu, "mu"), vec(resid, "resid")
    if not np.all((muv > 0.0) & (muv < 1.0)):
        raise ValueError("%s: every mu must lie in (0, 1)" % who)
    if not np.all(np.isfinite(rv)):
        raise ValueError("%s: resid must be finite" % who)
    Xa = np.asarray(X)
    if Xa.dtype.kind not in "iuf" or Xa.ndim != 2 or Xa.shape[0] != n or not 1 <= Xa.shape[1] <= SPA_MAX_COVARIATES:
        raise ValueError("%s: X must be numeric (%d, c) with 1 <= c <= %d, the intercept column included" % (who, n, SPA_MAX_COVARIATES))
    Xf = np.require(np.asarray(Xa, dtype=np.float64), requirements=["F", "ALIGNED"])
    if not np.all(np.isfinite(Xf)):
        raise ValueError("%s: X must be finite" % who)
    c = Xf.shape[1]
    if A is None:
        Am = np.linalg.inv(Xf.T @ ((muv * (1.0 - muv))[:, None] * Xf))
    else:
        Am = np.asarray(A)
        if Am.dtype.kind not in "iuf" or Am.shape != (c, c):
            raise ValueError("%s: A must be the (%d, %d) matrix (X'DX)^-1" % (who, c, c))
    Am = np.require(np.asarray(Am, dtype=np.float64), requirements=["F", "ALIGNED"])
    if not np.all(np.isfinite(Am)):
        raise ValueError("%s: A must be finite (collinear columns of X?)" % who)
    va = None
    if vara is not None:
        va = np.asarray(vara)
        if va.dtype.kind not in "iuf" or va.size != nm:
            raise ValueError("%s: vara must hold one number per marker (%d)" % (who, nm))
        va = np.ascontiguousarray(va.ravel(), dtype=np.float64)
    if isinstance(cutoff, bool) or not float(cutoff) >= 0.0:
        raise ValueError("%s: cutoff must be >= 0" % who)
    if not 0.0 < float(tol) < 1.0:
        raise ValueError("%s: tol must lie in (0, 1)" % who)
    if int(max_iter) != max_iter or not 1 <= max_iter <= 1000:
        raise ValueError("%s: max_iter must be a whole number in [1, 1000]" % who)
    return muv, rv, Xf, Am, va


def spa(f_name_ascii_Mt, dims, mu, resid, X, A=None, vara=None, cutoff=2.0, tol=1e-10, max_iter=50, availmemGb=8, device=0):
    """eagle_glmm_spa -> (stat fp64 (L, 7) = (T, V*, z, zeta_up, r*_up, zeta_lo, r*_lo), info int32 (L, 2) = (code, evaluations)) for every
    marker of Mt.ascii (dims = (n, L) of M; g = 0, 1, 2 copies of the '2' character) by the rule of include/eagle_hip.h section 1d''':
    mu and resid = y - mu of the null fit (n), X (n, c <= 15; the caller supplies the intercept), A = (X'DX)^-1 (formed here when None),
    vara = m' P m per marker (None: V = V*).  Codes: 0 both tails solved, 1 max_iter, 2 degenerate marker, 3 the observed statistic is
    at the edge of its support, 4 |z| <= cutoff (no saddlepoint taken), + 256 the opposite tail has no mass.  With a view alias the
    operands hold one entry per kept individual.  spa_host restates it; spa_pvalues makes the p-values."""
    n, nm = int(dims[0]), int(dims[1])
    muv, rv, Xf, Am, va = _spa_inputs("spa", n, nm, mu, resid, X, A, vara, cutoff, tol, max_iter)
    from . import rcpp_api
    L = _lib.load()
    stat, info = np.zeros((nm, 7), dtype=np.float64), np.zeros((nm, 2), dtype=np.int32)
    dp = rcpp_api._dp
    rcpp_api._args_first(L.eagle_glmm_spa, device, (os.fsencode(f_name_ascii_Mt), rcpp_api._dims((n, nm)), dp(muv), dp(rv), dp(Xf), Xf.shape[1],
                                                    dp(Am), None if va is None else dp(va), float(cutoff), float(tol), int(max_iter),
                                                    float(availmemGb), dp(stat), info.ctypes.data_as(C.POINTER(C.c_int32))))
    return stat, info


def _cgf(zeta, gt, mu, D):
    """(K, K', K'') of section 1d''' 4 at zeta."""
    a = zeta * gt
    ab = np.abs(a)
    nu = np.where(a >= 0.0, 1.0 - mu, mu)
    e = np.exp(-ab)
    u = 1.0 - e
    inv = 1.0 / (1.0 - nu * u)
    dgt = D * gt
    return (float(np.sum(nu * ab + np.log1p(-nu * u))), float(np.sum(np.where(a >= 0.0, dgt, -dgt) * u * inv)),
            float(np.sum(dgt * gt * e * inv * inv)))


def _tail(target, sgn, zmax, Vs, gt, mu, D, tol, max_iter):
    """One tail of section 1d''' 5 and 6 -> (zeta, r*, code, evaluations); code 5 = unreachable."""
    nan = float("nan")
    lo, hi = 0.0, sgn * zmax
    K0, K1, K2 = _cgf(hi, gt, mu, D)
    used = 1
    if not sgn * (K1 - target) > SPA_DEGENERATE * abs(target):
        return nan, nan, 5, used
    rv = math.sqrt(Vs)
    zeta, f, k2, K0 = 0.0, -target, Vs, 0.0
    while True:
        with np.errstate(all="ignore"):
            zn = zeta - f / k2 if k2 != 0.0 else nan
        if not (sgn * (zn - lo) >= 0.0 and sgn * (hi - zn) >= 0.0):
            zn = 0.5 * (lo + hi)
        delta = zn - zeta
        zeta = zn
        if used >= max_iter:
            return nan, nan, 1, used
        K0, K1, k2 = _cgf(zeta, gt, mu, D)
        used += 1
        f = K1 - target
        if sgn * f > 0.0:
            hi = zeta
        else:
            lo = zeta
        if abs(delta) * rv <= tol:
            break
    if abs(zeta) * rv < SPA_NEAR_ZERO:
        return zeta, target / rv, 0, used
    with np.errstate(all="ignore"):
        w = sgn * np.sqrt(2.0 * (zeta * target - K0))
        v = zeta * np.sqrt(k2)
        return zeta, float(w + np.log(v / w) / w), 0, used


def spa_host(Mt8, mu, resid, X, A=None, vara=None, cutoff=2.0, tol=1e-10, max_iter=50):
    """spa restated in numpy, marker by marker: Mt8 = int8 (L, n) of -1 / 0 / +1 (marker-major) -> (stat (L, 7), info (L, 2)) by the rule
    of include/eagle_hip.h section 1d'''.  Not bit-equal to the device (exp, log1p and the order of the sums differ);
    tests/glmm_truth.py holds both to 40-digit roots."""
    G = np.asarray(Mt8)
    nm, n = G.shape
    muv, rv, Xf, Am, va = _spa_inputs("spa_host", n, nm, mu, resid, X, A, vara, cutoff, tol, max_iter)
    D = muv * (1.0 - muv)
    nan, inf = float("nan"), float("inf")
    stat, info = np.full((nm, 7), nan), np.zeros((nm, 2), dtype=np.int32)
    for m in range(nm):
        g = G[m].astype(np.float64) + 1.0
        beta = Am @ (Xf.T @ (D * g))
        gt = g - Xf @ beta
        T, Vs, S2 = float(g @ rv), float(np.sum(D * gt * gt)), float(np.sum(D * g * g))
        stat[m, :2] = T, Vs
        V = Vs if va is None else float(va[m])
        if not Vs > SPA_DEGENERATE * S2 or not (V > 0.0 and V < inf):
            info[m] = 2, 0
            continue
        z = T / math.sqrt(V)
        q = z * math.sqrt(Vs)
        stat[m, 2] = z
        if abs(z) <= cutoff:
            info[m] = 4, 0
            continue
        aq, zmax = abs(q), SPA_ZETA_RANGE / float(np.max(np.abs(gt)))
        up = T > 0.0
        s1 = 1.0 if up else -1.0
        z1, r1, c1, ev = _tail(s1 * aq, s1, zmax, Vs, gt, muv, D, tol, max_iter)
        if c1:
            info[m] = (3 if c1 == 5 else c1), ev
            continue
        z2, r2, c2, e2 = _tail(-s1 * aq, -s1, zmax, Vs, gt, muv, D, tol, max_iter)
        ev += e2
        code = c2
        if c2 == 5:
            code, z2, r2 = 256, -s1 * zmax, -s1 * inf
        info[m] = code, ev
        if code & 255 == 0:
            stat[m, 3:] = (z1, r1, z2, r2) if up else (z2, r2, z1, r1)
    return stat, info


def spa_pvalues(stat, info):
    """{"p_norm": 2 Phi(-|z|), "p_spa": Phi(-r*_up) + Phi(r*_lo) (NaN unless the code's low byte is 0), "p": p_spa where it exists and
    p_norm elsewhere, "spa_used"} of a (stat, info) that spa or spa_host returned."""
    from scipy.special import ndtr
    stat, code = np.asarray(stat, dtype=np.float64), np.asarray(info)[:, 0]
    with np.errstate(all="ignore"):
        p_norm = 2.0 * ndtr(-np.abs(stat[:, 2]))
        p_spa = ndtr(-stat[:, 4]) + ndtr(stat[:, 6])
    used = (code & 255) == 0
    p_spa = np.where(used, p_spa, np.nan)
    return {"p_norm": p_norm, "p_spa": p_spa, "p": np.where(used, p_spa, p_norm), "spa_used": used}


# ---------------------------------------------------------------------------------------------------------------------------
# The null model
# ---------------------------------------------------------------------------------------------------------------------------
class _Working:
    """The working linear model Y ~ N(X alpha, D^-1 + tau K) of one PQL step in the eigenbasis of D^1/2 K D^1/2 = Q diag(lam) Q'
    (the decomposition host_model.ZModel uses): Sigma^-1 = D^1/2 Q diag(1 / (1 + tau lam)) Q' D^1/2 for every tau from one eigh."""

    def __init__(self, K, X, Y, D):
        self.sd = np.sqrt(D)
        self.lam, self.Q = host_model.algebra().eigh(self.sd[:, None] * K * self.sd[None, :])
        self.lam = np.maximum(np.asarray(self.lam, dtype=np.float64), 0.0)          # K is positive semi-definite
        self.Xt, self.Yt = self.Q.T @ (self.sd[:, None] * X), self.Q.T @ (self.sd * Y)

    def gls(self, tau):
        w = 1.0 / (1.0 + tau * self.lam)
        WX = w[:, None] * self.Xt
        Cm = self.Xt.T @ WX
        alpha = np.linalg.solve(Cm, WX.T @ self.Yt)
        return w, WX, Cm, alpha, self.Yt - self.Xt @ alpha

    def reml(self, tau):
        """The REML criterion with dispersion 1, up to a constant that does not depend on tau."""
        w, _, Cm, _, e = self.gls(tau)
        return 0.5 * float(np.sum(np.log(w))) - 0.5 * float(np.linalg.slogdet(Cm)[1]) - 0.5 * float(np.sum(w * e * e))

    def score(self, tau):
        """1/2 Y'PKPY - 1/2 tr(PK)."""
        w, WX, Cm, _, e = self.gls(tau)
        wl = w * self.lam
        tr = float(np.sum(wl)) - float(np.trace(np.linalg.solve(Cm, WX.T @ (wl[:, None] * self.Xt))))
        return 0.5 * float(np.sum(wl * w * e * e)) - 0.5 * tr

    def best_tau(self):
        """The maximiser of reml over {0} + [e^-10, e^10]: a grid in ln tau, then the root of the score between the best point's
        neighbours."""
        from scipy.optimize import brentq
        th = np.linspace(-10.0, 10.0, 81)
        ll = np.array([self.reml(math.exp(t)) for t in th])
        i = int(np.argmax(ll))
        if self.reml(0.0) >= ll[i]:
            return 0.0
        lo, hi = th[max(i - 1, 0)], th[min(i + 1, th.size - 1)]
        f = lambda t: self.score(math.exp(t))                                       # noqa: E731
        if f(lo) > 0.0 > f(hi):
            return math.exp(brentq(f, lo, hi, xtol=1e-13, rtol=8.9e-16))
        return math.exp(th[i])                                                      # an end of the domain

    def solve(self, tau):
        """(alpha, b = tau K Sigma^-1 (Y - X alpha)) at tau."""
        w, _, _, alpha, e = self.gls(tau)
        return alpha, (self.Q @ (tau * self.lam * w * e)) / self.sd                 # K D^1/2 Q = D^-1/2 Q diag(lam)

    def projection(self, tau):
        """P = Sigma^-1 - Sigma^-1 X (X'Sigma^-1 X)^-1 X'Sigma^-1 (n x n) and P Y."""
        la = host_model.algebra()
        w, WX, Cm, _, e = self.gls(tau)
        QW = self.sd[:, None] * self.Q
        SX = QW @ WX                                                                # Sigma^-1 X
        P = np.asarray(la.mm(QW * w[None, :], QW.T)) - SX @ np.linalg.solve(Cm, SX.T)
        return 0.5 * (P + P.T), QW @ (w * e)


def null_fit(y, X, K, tau=None, tol=1e-6, max_iter=100):
    """The null logistic mixed model  logit mu_i = x_i' alpha + b_i, b ~ N(0, tau K)  of y (n, 0 / 1) on X (n x c, the intercept
    column included) and the kinship K (n x n), by penalised quasi-likelihood as GMMAT fits it.  One step, given (alpha, b):
    eta = X alpha + b, mu = expit(eta), D = diag(mu (1 - mu)), the working vector Y = eta + (y - mu) / D, Sigma = D^-1 + tau K;
    tau maximises the REML criterion of the working model with dispersion 1 over {0} + [e^-10, e^10] (tau= fixes it; 0.0 works);
    alpha <- (X'Sigma^-1 X)^-1 X'Sigma^-1 Y, b <- tau K Sigma^-1 (Y - X alpha).  From r_api.logistic_null_host and b = 0 until the
    largest change of eta is <= tol.

    At the fixed point alpha is the GLS estimate, b = tau K Sigma^-1 (Y - X alpha), 1/2 Y'PKPY - 1/2 tr(PK) = 0 for an interior tau
    (<= 0 at tau = 0, >= 0 at e^10), and y - mu = P Y, X'(y - mu) = 0.

    -> {"alpha", "b", "tau", "mu", "eta", "D", "converged", "iterations", "P" (n x n), "PY" (n), "Y", "A" = (X'DX)^-1}; P and PY are
    the operands of the scan (rcpp_api.scan_with_W(W = P, v = PY)), evaluated at the returned eta and tau."""
    from . import r_api
    yv = np.asarray(y, dtype=np.float64).ravel()
    Xa = np.asarray(X, dtype=np.float64)
    Xa = Xa[:, None] if Xa.ndim == 1 else Xa
    Km = np.asarray(K, dtype=np.float64)
    n = yv.size
    if Xa.ndim != 2 or Xa.shape[0] != n or Km.shape != (n, n):
        raise ValueError("null_fit: X must be (n, c) and K (n, n) for the n = %d entries of y" % n)
    if not np.all((yv == 0.0) | (yv == 1.0)) or not (yv == 1.0).any() or not (yv == 0.0).any():
        raise ValueError("null_fit: y must hold 0 and 1, both present")
    if not np.all(np.isfinite(Xa)) or not np.all(np.isfinite(Km)):
        raise ValueError("null_fit: X and K must be finite")
    if tau is not None and not (float(tau) == 0.0 or TAU_MIN <= float(tau) <= TAU_MAX):
        raise ValueError("null_fit: tau must be 0 or lie in [e^-10, e^10]")
    if not 0.0 < float(tol) < 1.0 or int(max_iter) < 1:
        raise ValueError("null_fit: tol must lie in (0, 1) and max_iter be at least 1")
    alpha = r_api.logistic_null_host(Xa, yv)
    eta = Xa @ alpha
    t, converged, it = (0.0 if tau is None else float(tau)), False, 0
    while it < int(max_iter):
        it += 1
        mu = _expit(eta)
        D = mu * (1.0 - mu)
        wm = _Working(Km, Xa, eta + (yv - mu) / D, D)
        if tau is None:
            t = wm.best_tau()
        alpha, b = wm.solve(t)
        new = Xa @ alpha + b
        change = float(np.max(np.abs(new - eta)))
        eta = new
        if change <= tol:
            converged = True
            break
    mu = _expit(eta)
    D = mu * (1.0 - mu)
    Y = eta + (yv - mu) / D
    wm = _Working(Km, Xa, Y, D)
    P, PY = wm.projection(t)
    return {"alpha": alpha, "b": eta - Xa @ alpha, "tau": t, "mu": mu, "eta": eta, "D": D, "converged": converged, "iterations": it, "P": P,
            "PY": PY, "Y": Y, "A": np.linalg.inv(Xa.T @ (D[:, None] * Xa))}


def _expit(eta):
    e = np.exp(-np.abs(eta))
    return np.where(eta >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


# ---------------------------------------------------------------------------------------------------------------------------
# The analysis
# ---------------------------------------------------------------------------------------------------------------------------
def _status(who, status, n):
    st = list(np.asarray(status, dtype=object).ravel())
    y = np.full(len(st), np.nan)
    for i, v in enumerate(st):
        if v is None or (isinstance(v, (float, np.floating)) and math.isnan(v)):
            continue
        if isinstance(v, (str, bytes)) or (v != 0 and v != 1):
            raise ValueError("%s: status must be 1 (case), 0 (control) or NaN / None (not used)" % who)
        y[i] = float(v)
    if y.size != n:
        raise ValueError("%s: %d status records for %d genotyped individuals" % (who, y.size, n))
    return y


def GLMM(geno, status, X=None, tau=None, spa_cutoff=2.0, tol=1e-10, max_iter=50, map=None, backend=None, availmemGb=8, device=0):
    """Case/control association of every marker of a panel under the logistic mixed model; r_api.GLMM forwards here.

    status (n): 1 = case, 0 = control, NaN / None = not used, as Logistic takes it.  X: (n, c <= 15) covariates WITH the intercept
    column; None = intercept only; an individual with a NaN covariate is not used.  The individuals not used leave the genotypes by a
    VIEW reshape, as AM() drops them.  K is the backend's (calcMMt: MM'/max + 0.95 I; backend: an am.HipBackend, default a new one on
    `device`), the null model is null_fit(y, X, K, tau), V_m = m' P m comes from one rcpp_api.scan_with_W(W = P, v = P Y) over the
    int8 image, and spa() turns every score into its saddlepoint deviates (cutoff spa_cutoff; tol and max_iter are the root
    search's).

    Returns a dict of fp64 (L) columns unless noted: "score" = T^2 / V, "p_norm" = chdtrc(1, score), "p_spa", "p" = p_spa where the
    code's low byte is 0 and p_norm elsewhere, "spa_used" (bool), "beta" = T / V (one scoring step, per copy of the '2' character's
    allele), "se" = 1 / sqrt(V), "code" and "evaluations" (int32; the codes of spa); "null": {"tau", "alpha", "converged",
    "iterations"}; "lambda_gc" = median(score) / 0.4549... (the chi^2_1 median), "n_used", "indxNA" and, with map= (L names or a
    mapping with "SNP"), "names".  There is no Zmat=: repeated measures are not supported."""
    from scipy.special import chdtri
    from . import am, r_api, rcpp_api
    n0, L = int(geno["dim_of_ascii_M"][0]), int(geno["dim_of_ascii_M"][1])
    y = _status("GLMM", status, n0)
    Xa = np.ones((n0, 1)) if X is None else np.asarray(X, dtype=np.float64)
    Xa = Xa[:, None] if Xa.ndim == 1 else Xa
    if Xa.ndim != 2 or Xa.shape[0] != n0 or not 1 <= Xa.shape[1] <= SPA_MAX_COVARIATES:
        raise ValueError("GLMM: X must be (%d, c) with 1 <= c <= %d, the intercept column included" % (n0, SPA_MAX_COVARIATES))
    if np.any(np.isinf(Xa)):
        raise ValueError("GLMM: X holds an infinite entry")
    if tau is not None and not (float(tau) == 0.0 or TAU_MIN <= float(tau) <= TAU_MAX):
        raise ValueError("GLMM: tau must be 0 or lie in [e^-10, e^10]")
    _spa_inputs("GLMM", 1, 1, [0.5], [0.0], np.ones((1, 1)), None, None, spa_cutoff, tol, max_iter)   # the search parameters
    y[np.isnan(Xa).any(axis=1)] = np.nan
    if not (y == 1.0).any() or not (y == 0.0).any():
        raise ValueError("GLMM: no case or no control among the used individuals")
    backend = backend or am.HipBackend(device)
    indxNA = r_api.check_for_NA_in_trait(y)
    (y, Xa), geno = am._drop_na_rows(indxNA, (y, Xa), geno, backend=backend, device=backend.device)
    n = int(geno["dim_of_ascii_M"][0])
    names = None if map is None else am._summary_names(Xa.shape[1], None, map, L)[1]
    K = backend.calcMMt(geno, availmemGb, 1, np.array([np.nan]), True)
    fit = null_fit(y, Xa, K, tau=tau)
    scan = rcpp_api.scan_with_W(geno["asciifileMt"], np.nan, fit["P"], fit["PY"], availmemGb, (L, n), device=backend.device)
    V = scan["vara"].ravel()
    stat, info = spa(geno["asciifileMt"], (n, L), fit["mu"], y - fit["mu"], Xa, fit["A"], V, spa_cutoff, tol, max_iter, availmemGb,
                     device=backend.device)
    out = glmm_columns(stat, info, V)
    out.update({"null": {k: fit[k] for k in ("tau", "alpha", "converged", "iterations")}, "n_used": n, "indxNA": indxNA,
                "lambda_gc": float(np.nanmedian(out["score"]) / chdtri(1.0, 0.5))})
    if names is not None:
        out["names"] = [names(j) for j in range(1, L + 1)]
    return out


def glmm_columns(stat, info, V):
    """The per-marker columns of GLMM from spa's (stat, info) and the V it was given."""
    T, z = stat[:, 0], stat[:, 2]
    bad = info[:, 0] == 2
    with np.errstate(all="ignore"):
        Vm = np.where(bad, np.nan, V)
        out = {"score": z * z, "beta": T / Vm, "se": 1.0 / np.sqrt(Vm), "code": info[:, 0].copy(), "evaluations": info[:, 1].copy()}
    out.update(spa_pvalues(stat, info))
    return out
