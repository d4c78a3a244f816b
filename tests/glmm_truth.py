"""40-digit truth for the saddlepoint rule of include/eagle_hip.h section 1d''' (mpmath), the allowance the fp64 implementations get
against it, and the fixtures tests/test_glmm_host.py and tests/test_gpu_glmm.py share.

truth(mu, X, g, resid, V) takes the SAME fp64 operands the implementations take and evaluates the rule -- G~, T, V*, q, the roots of
K' = +-|q|, r*, p -- at 40 digits, with the exact sums sum log(1 - mu + mu e^(t G~)) - t m etc. of the header's first form, not the
rearranged terms the implementations use.

The allowance on ln p (allowance()) has two parts, neither taken from the code under test.

  1. The stop rule's share.  The search ends when a step |delta zeta| sqrt(V*) <= tol; a Newton step overestimates the distance to the
     root once it converges and a bisection step equals the half width of the bracket, so the root is within tol / sqrt(V*) of the
     zeta returned.  ln p moves by |d ln p / d zeta| times that, d ln p / d zeta = sum over the tails of phi(r*) |dr*/dzeta| / p, the
     derivative taken at 40 digits (dlnp_dzeta).

  2. Rounding, to first order.  A sum of n fp64 terms carries at most n 2^-53 times the sum of its terms' magnitudes (any order of
     summation).  With M0, M1, M2 the magnitude sums of the terms of K, K', K'' and h_i = |g_i| + sum_j |x_ij beta_j| the magnitude of
     G~_i's own terms (whose rounding moves a term of K by at most |zeta| h_i, of K' by (1 + |a_i|) h_i and of K'' by
     2 |G~_i| (1 + |a_i|) h_i D_i: the derivatives of the three terms in G~, bounded), the errors and what they do to r* are
         K':  the root moves by dK' / K'', the target tau = +-|q| by |tau| Tq, Tq = sum |g_i r_i| / |T| + 1 (T, and V* / V under the root):
                  |dr*/dzeta| (M1 + |tau| Tq) / K'';
         K and tau in w = sqrt(2 (zeta tau - K)):  dw = (dK + |zeta tau| Tq) / |w|, and dr*/dw = 1 - (ln(v / w) + 1) / w^2;
         K'' in v = zeta sqrt(K''):  dr* = (1 / |w|) dK'' / (2 K'');
     each times phi(r*) / p for ln p.  Where the rule takes r* = tau / sqrt(V*) the only error is tau's: |r*| Tq.
     ROUNDING_FACTOR = 4 multiplies n 2^-53 times that sum: 1 for the sums themselves, and 3 for what the bound above leaves out
     -- exp and log1p are good to a few ulp, not half of one, and each term is a product of up to six rounded operations.
     With n <= 257 this part is some 1e-13 on ln p: the stop rule's share at tol = 1e-10 dominates, and the measured headroom
     is large because Newton's last step overestimates its error by orders of magnitude.
"""
import hashlib

import mpmath as mp
import numpy as np

DPS = 40
ROUNDING_FACTOR = 4.0
DEGENERATE, ZETA_RANGE, NEAR_ZERO = mp.mpf(2) ** -40, mp.mpf(500), mp.mpf("1e-4")
_cache = {}


def _phi(x):
    return mp.npdf(x)


class _Marker:
    """The 40-digit operands of one marker."""

    def __init__(self, mu, X, g, resid, V, A):
        f = lambda a: [mp.mpf(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()]   # noqa: E731
        self.n = len(mu)
        self.mu, self.g, self.r = f(mu), f(g), f(resid)
        Xa = np.asarray(X, dtype=np.float64)
        self.c = Xa.shape[1]
        self.X = [[mp.mpf(float(v)) for v in row] for row in Xa]
        self.D = [m * (1 - m) for m in self.mu]
        if A is None:
            XtDX = mp.matrix(self.c, self.c)
            for i in range(self.n):
                for a in range(self.c):
                    for b in range(self.c):
                        XtDX[a, b] += self.D[i] * self.X[i][a] * self.X[i][b]
            Am = XtDX ** -1
        else:
            Am = mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(A, dtype=np.float64)])
        s = [mp.fsum(self.D[i] * self.g[i] * self.X[i][a] for i in range(self.n)) for a in range(self.c)]
        self.beta = [mp.fsum(Am[a, b] * s[b] for b in range(self.c)) for a in range(self.c)]
        self.gt = [self.g[i] - mp.fsum(self.X[i][a] * self.beta[a] for a in range(self.c)) for i in range(self.n)]
        self.h = [abs(self.g[i]) + mp.fsum(abs(self.X[i][a] * self.beta[a]) for a in range(self.c)) for i in range(self.n)]
        self.T = mp.fsum(self.g[i] * self.r[i] for i in range(self.n))
        self.Tmag = mp.fsum(abs(self.g[i] * self.r[i]) for i in range(self.n))
        self.Vs = mp.fsum(self.D[i] * self.gt[i] ** 2 for i in range(self.n))
        self.S2 = mp.fsum(self.D[i] * self.g[i] ** 2 for i in range(self.n))
        self.m = mp.fsum(self.gt[i] * self.mu[i] for i in range(self.n))
        self.V = self.Vs if V is None else mp.mpf(float(V))

    def K(self, t):
        return mp.fsum(mp.log(1 - self.mu[i] + self.mu[i] * mp.exp(t * self.gt[i])) for i in range(self.n)) - t * self.m

    def K1(self, t):
        return mp.fsum(self.mu[i] * self.gt[i] / ((1 - self.mu[i]) * mp.exp(-t * self.gt[i]) + self.mu[i]) for i in range(self.n)) - self.m

    def K2(self, t):
        out = []
        for i in range(self.n):
            e = mp.exp(-t * self.gt[i])
            out.append((1 - self.mu[i]) * self.mu[i] * self.gt[i] ** 2 * e / ((1 - self.mu[i]) * e + self.mu[i]) ** 2)
        return mp.fsum(out)

    def magnitudes(self, t):
        """(M0, M1, M2) of the module docstring at t: the centred per-individual terms the implementations sum, plus G~'s rounding."""
        M0 = M1 = M2 = mp.mpf(0)
        for i in range(self.n):
            a = t * self.gt[i]
            e = mp.exp(-a)
            den = (1 - self.mu[i]) * e + self.mu[i]
            k0 = mp.log(1 - self.mu[i] + self.mu[i] * mp.exp(a)) - self.mu[i] * a
            k1 = self.mu[i] * self.gt[i] / den - self.mu[i] * self.gt[i]
            k2 = self.D[i] * self.gt[i] ** 2 * e / den ** 2
            M0 += abs(k0) + abs(t) * self.h[i]
            M1 += abs(k1) + (1 + abs(a)) * self.h[i]
            M2 += k2 + 2 * abs(self.gt[i]) * (1 + abs(a)) * self.h[i] * self.D[i]
        return M0, M1, M2

    def rstar(self, zeta, tau):
        w = mp.sign(zeta) * mp.sqrt(2 * (zeta * tau - self.K(zeta)))
        v = zeta * mp.sqrt(self.K2(zeta))
        return w + mp.log(v / w) / w

    def tail(self, tau, sgn, zmax):
        """-> dict(reachable, zeta, rstar, drdz, round) for the target tau."""
        if not sgn * (self.K1(sgn * zmax) - tau) > DEGENERATE * abs(tau):
            return {"reachable": False}
        lo, hi = mp.mpf(0), sgn * zmax
        zeta = tau / self.Vs
        for _ in range(400):                                                   # safeguarded Newton at 40 digits
            if not (sgn * (zeta - lo) > 0 and sgn * (hi - zeta) > 0):
                zeta = (lo + hi) / 2
            f = self.K1(zeta) - tau
            if sgn * f > 0:
                hi = zeta
            else:
                lo = zeta
            step = f / self.K2(zeta)
            zeta -= step
            if abs(step) <= abs(zeta) * mp.mpf(10) ** (-DPS + 6):
                break
        else:
            raise AssertionError("the 40-digit root search did not converge")
        rv = mp.sqrt(self.Vs)
        Tq = self.Tmag / abs(self.T) + 1
        if abs(zeta) * rv < NEAR_ZERO:
            r = tau / rv
            return {"reachable": True, "zeta": zeta, "rstar": r, "drdz": mp.mpf(0), "round": abs(r) * Tq}
        r = self.rstar(zeta, tau)
        drdz = mp.diff(lambda t: self.rstar(t, tau), zeta)
        K2 = self.K2(zeta)
        w = mp.sign(zeta) * mp.sqrt(2 * (zeta * tau - self.K(zeta)))
        v = zeta * mp.sqrt(K2)
        M0, M1, M2 = self.magnitudes(zeta)
        rnd = (abs(drdz) * (M1 + abs(tau) * Tq) / K2 + abs(1 - (mp.log(v / w) + 1) / w ** 2) * (M0 + abs(zeta * tau) * Tq) / abs(w)
               + M2 / (2 * abs(w) * K2))
        return {"reachable": True, "zeta": zeta, "rstar": r, "drdz": drdz, "round": rnd}


def truth(mu, X, g, resid, V=None, A=None, cutoff=0.0):
    """The rule at 40 digits for one marker with allele counts g (n, values 0 / 1 / 2) -> dict: code (as the rule reports it, max_iter
    aside), T, Vs, z, p_norm, and where the saddlepoint is taken zeta_up, r_up, zeta_lo, r_lo, p, lnp, dlnp_dzeta (the sum of both
    tails' |d ln p / d zeta|) and lnp_round (the bracket of the docstring's part 2, to be multiplied by ROUNDING_FACTOR n 2^-53).
    Floats, except that nothing is rounded before p is formed."""
    key = hashlib.sha256(b"".join(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes() for a in
                                  (mu, X, g, resid, [np.nan if V is None else V], [np.nan] if A is None else A, [cutoff]))).hexdigest()
    if key in _cache:
        return _cache[key]
    with mp.workdps(DPS):
        M = _Marker(mu, X, g, resid, V, A)
        out = {"T": float(M.T), "Vs": float(M.Vs), "n": M.n}
        if not M.Vs > DEGENERATE * M.S2 or not (mp.isfinite(M.V) and M.V > 0):
            out["code"] = 2
        else:
            z = M.T / mp.sqrt(M.V)
            q = z * mp.sqrt(M.Vs)
            out.update({"z": float(z), "p_norm": float(2 * mp.ncdf(-abs(z)))})
            if abs(z) <= cutoff:
                out["code"] = 4
            else:
                zmax = ZETA_RANGE / max(abs(v) for v in M.gt)
                up, lo = M.tail(abs(q), 1, zmax), M.tail(-abs(q), -1, zmax)
                obs, opp = (up, lo) if M.T > 0 else (lo, up)
                if not obs["reachable"]:
                    out["code"] = 3
                else:
                    out["code"] = 0 if opp["reachable"] else 256
                    p_up = mp.ncdf(-up["rstar"]) if up["reachable"] else mp.mpf(0)
                    p_lo = mp.ncdf(lo["rstar"]) if lo["reachable"] else mp.mpf(0)
                    p = p_up + p_lo
                    sens = sum(_phi(t["rstar"]) * abs(t["drdz"]) for t in (up, lo) if t["reachable"]) / p
                    rnd = sum(_phi(t["rstar"]) * t["round"] for t in (up, lo) if t["reachable"]) / p
                    out.update({"p": float(p), "lnp": float(mp.log(p)), "dlnp_dzeta": float(sens), "lnp_round": float(rnd),
                                "zeta_up": float(up["zeta"]) if up["reachable"] else float(zmax),
                                "zeta_lo": float(lo["zeta"]) if lo["reachable"] else float(-zmax),
                                "r_up": float(up["rstar"]) if up["reachable"] else float("inf"),
                                "r_lo": float(lo["rstar"]) if lo["reachable"] else float("-inf")})
    _cache[key] = out
    return out


def allowance(t, tol):
    """What |ln p - the truth's| may be for an implementation run with the stop rule tol (module docstring, parts 1 and 2)."""
    return t["dlnp_dzeta"] * tol / np.sqrt(t["Vs"]) + ROUNDING_FACTOR * t["n"] * 2.0 ** -53 * t["lnp_round"]


def lnp_of(stat_row):
    """ln p_spa of one row of spa's stat, formed in log space so that a far tail keeps its digits."""
    from scipy.special import log_ndtr
    return float(np.logaddexp(log_ndtr(-stat_row[4]), log_ndtr(stat_row[6])))


# ---- the fixtures both test files use -------------------------------------------------------------------------------------------
def covariates(n, c, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])


def panel(n, L, c, seed, prevalence=0.05, maf=0.04):
    """(Mt8 int8 (L, n), mu, resid, X, vscale (L)): operands with mu around `prevalence` and rare alleles.  With c = 1 mu is the
    intercept-only fit itself (the mean of y); with covariates it is the model's mu, not a fit (the rule takes any mu and resid).  The
    implementations get vara = vscale * V*.  Planted at the end when L >= 5:
      L-1 monomorphic (code 2);
      L-2 five carriers with the smallest mu, four of them cases: a large |z|, and with c = 4 an opposite tail without mass (+ 256);
      L-3 a common marker (|z| small: code 4 at cutoff 2);
      L-4 the carriers are exactly the cases and vscale = 0.8 puts |q| beyond the support (code 3)."""
    rng = np.random.default_rng(seed)
    X = covariates(n, c, seed + 1)
    eta = np.log(prevalence / (1 - prevalence)) + (0.4 * (X[:, 1:] @ rng.standard_normal(c - 1)) / np.sqrt(c - 1) if c > 1 else np.zeros(n))
    mu = 1.0 / (1.0 + np.exp(-eta))
    y = (rng.random(n) < mu).astype(np.float64)
    order = np.argsort(mu, kind="stable")
    y[order[:min(4, n - 3)]] = 1.0
    y[order[-2:]] = 1.0
    y[order[-3]] = 0.0
    if c == 1:
        mu = np.full(n, y.mean())
    G = rng.binomial(2, maf, size=(L, n))
    for m in range(L):                                                         # no marker without a carrier
        if G[m].sum() == 0:
            G[m, rng.integers(n)] = 1
    vscale = np.ones(L)
    if L >= 5:
        G[L - 1] = 0
        G[L - 2] = 0
        G[L - 2, order[:min(5, n - 2)]] = 1
        G[L - 3] = rng.binomial(2, 0.4, size=n)
        G[L - 4] = y.astype(np.int64)
        vscale[L - 4] = 0.8
    return (G - 1).astype(np.int8), mu, y - mu, X, vscale
