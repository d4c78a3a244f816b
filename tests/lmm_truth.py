"""Truth for the exact mixed-model test of include/eagle_hip.h section 1d', in mpmath at 40 digits: per marker the root theta* of
g(theta) = delta l'(delta) reached from theta0 by the header's safeguarded outline (Newton inside a sign bracket, steps of at most 2,
bisection, the limits -10 and 10), REML and ML, both written here from the model alone -- nothing is shared with r_api.lmm_host or the
kernel but the model -- then gamma, se and l at the root and the numbers the error bounds need: |g'(theta*)|, cond(A_1), the
derivatives of gamma and se in theta, and first-order bounds of what rounding does to g, gamma, se and l (below).

The panels of tests/test_lmm_host.py and tests/test_gpu_lmm.py are defined here (panel()): K = G G' / max + 0.95 I of a seeded random
genotype matrix, as AM() forms it; the tested markers are the first L of panel()'s G; the trait is X b + one planted marker + a polygenic part made
of integer marker effects + noise.  Everything the digest covers (G, X, y) is made of integers and elementwise fp64 operations, so
every machine makes the same bits; lam, U = eigh(K) are not, and need not be: the model -- and so the truth -- depends on K, X, y and
the marker alone, not on the basis K is diagonalised in, and what a basis rounded differently does to g enters like the rounding of
the sums that the bounds already carry (bounds()).

The truth costs minutes of mpmath, so it is computed once (`python tests/lmm_truth.py` rewrites tests/golden/lmm_truth.npz) and keyed
by a digest of each panel's inputs: golden() refuses a file made from other inputs, and tests/test_lmm_host.py recomputes entries live.

Rounding bounds, all to first order in eps = 8 (n + 16) 2^-53 (the constant of tests/logistic_truth.py: a term of a sum S_r carries
the roundings of e^theta, one division, w^2, w^3, two products and its place in a sum of n).  With |S|_r = sum_k w_k^r |B_ka| |B_kb|
the entrywise bound of S_r's error per unit eps, v = (beta, -1) so that R = v' S_1 v and Q = v' S_2 v, u = b_2 - A_2 beta,
h = A_1^-1 u and Inv = A_1^-1:
    dR     = |v|' |S|_1 |v|                                  (beta minimises R: its own error enters R only to second order)
    dQ     = |v|' |S|_2 |v| + 2 |h|' |S|_1[:p, :] |v|        (dQ/dbeta = -2 u, dbeta = -Inv [dS_1 v]_1..p)
    dT     = s_1 + sum |Inv| o |A|_2 + sum |Inv A_2 Inv| o |A|_1         (REML; ML: s_1)
    round_g     = delta / 2 [m dQ / R + m Q dR / R^2 + dT] + cond(A_1) delta / 2 [2 m |u|' |beta| / R + sum |Inv| o |A_2|]
    round_gamma = sum_b |Inv_pb| (|S|_1 |v|)_b + cond(A_1) max |beta|
    round_se    = 1/2 [dR / R + |Inv_p|' |A|_1 |Inv_p| / Inv_pp + cond(A_1)]                            (relative)
    round_ll    = 1/2 [m dR / R + sum_k |log w_k| + p cond(A_1)]
the cond(A_1) terms standing for the Cholesky solves, whose error is a few p 2^-53 cond(A_1) relative."""
import hashlib
import math
import os

import mpmath
import numpy as np

DPS = 40
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lmm_truth.npz")
NS = [20, 63, 64, 65, 255, 256, 257, 1003]
LS = [1, 3, 4, 5, 129]
CS = [1, 2, 4, 14]
LLIM, ULIM, STEP_MAX = -10, 10, 2
PIVOT_CLEAR = 2.0 ** -30      # the rule calls a pivot singular below 2^-40 of its diagonal entry: a clear marker keeps a margin of 2^10
# One seed per panel, chosen (`python tests/lmm_truth.py seeds`) as the first of base, base + 1000, ... for which at least 90 % of the markers are
# clear under both methods in the mpmath truth; tests/test_lmm_host.py asserts that they are.
SEEDS = {"n20": 363020, "n63": 12063, "n64": 12064, "n65": 19065, "n255": 11255, "n256": 11256, "n257": 11257, "n1003": 12003, "L1": 16001,
         "L3": 15003, "L4": 14004, "L5": 12005, "L129": 14129, "c1": 14001, "c2": 23002, "c4": 17004, "c14": 25014}
FIELDS = ("clear", "code", "theta", "gamma", "se", "ll", "gp", "cond", "d_gamma", "d_se", "round_g", "round_gamma", "round_se", "round_ll")
U53 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the model in mpmath
class _Marker:
    """B = [U^T X | z | U^T y] of one marker as mpf, with the products B_ka B_kb formed once."""

    def __init__(self, lam, UtX, Uty, z):
        B = np.column_stack([np.asarray(UtX, dtype=np.float64).reshape(len(lam), -1), z, Uty])
        self.n, self.P = B.shape
        self.p = self.P - 1
        self.lam = [mpmath.mpf(float(v)) for v in lam]
        cols = [[mpmath.mpf(float(v)) for v in B[:, a]] for a in range(self.P)]
        self.prod = {(a, b): [x * y for x, y in zip(cols[a], cols[b])] for a in range(self.P) for b in range(a + 1)}
        self.aprod = {k: [abs(x) for x in v] for k, v in self.prod.items()}

    def gram(self, wr, absolute=False):
        src = self.aprod if absolute else self.prod
        S = mpmath.zeros(self.P)
        for (a, b), v in src.items():
            S[a, b] = S[b, a] = mpmath.fdot(v, wr)
        return S

    def evaluate(self, theta, reml, full=False):
        """g, g' at theta and, with full=True, everything at_root() reports.  None: A_1 is singular at 40 digits."""
        p, n = self.p, self.n
        delta = mpmath.exp(theta)
        w = [1 / (l + delta) for l in self.lam]
        w2 = [x * x for x in w]
        w3 = [x * y for x, y in zip(w2, w)]
        S1, S2, S3 = self.gram(w), self.gram(w2), self.gram(w3)
        A1, A2, A3 = S1[:p, :p], S2[:p, :p], S3[:p, :p]
        b1, b2, b3 = S1[:p, p], S2[:p, p], S3[:p, p]
        try:
            Inv = A1 ** -1
        except ZeroDivisionError:
            return None
        beta = Inv * b1
        dot = lambda x, y: mpmath.fsum(x[i] * y[i] for i in range(p))
        R = S1[p, p] - dot(b1, beta)
        Q = S2[p, p] - 2 * dot(beta, b2) + dot(beta, A2 * beta)
        u = b2 - A2 * beta
        C = S3[p, p] - 2 * dot(beta, b3) + dot(beta, A3 * beta) - dot(u, Inv * u)
        s1, s2 = mpmath.fsum(w), mpmath.fsum(w2)
        if reml:
            M = Inv * A2
            m = n - p
            T = s1 - mpmath.fsum(M[i, i] for i in range(p))
            M3 = Inv * A3
            T2 = s2 - 2 * mpmath.fsum(M3[i, i] for i in range(p)) + mpmath.fsum(M[i, j] * M[j, i] for i in range(p) for j in range(p))
        else:
            m, T, T2 = n, s1, s2
        lp = (m * Q / R - T) / 2
        lpp = (m * (Q * Q / (R * R) - 2 * C / R) + T2) / 2
        g = delta * lp
        gp = g + delta * delta * lpp
        if not full:
            return g, gp
        ll = m * (mpmath.log(m / (2 * mpmath.pi)) - 1 - mpmath.log(R)) + mpmath.fsum(mpmath.log(x) for x in w)
        if reml:
            ll -= mpmath.log(mpmath.det(A1))
        gamma, ipp = beta[p - 1], Inv[p - 1, p - 1]
        se = mpmath.sqrt(R / m * ipp)
        # the first-order rounding bounds of the module docstring
        aS1, aS2 = self.gram(w, True), self.gram(w2, True)
        av = [abs(beta[i]) for i in range(p)] + [mpmath.mpf(1)]
        P = self.P
        quad = lambda x, S, y, rows: mpmath.fsum(x[a] * S[a, b] * y[b] for a in range(rows) for b in range(P))
        dR = quad(av, aS1, av, P)
        h = Inv * u
        dQ = quad(av, aS2, av, P) + 2 * quad([abs(h[i]) for i in range(p)], aS1, av, p)
        dT = s1
        A1f = np.array([[float(A1[i, j]) for j in range(p)] for i in range(p)])
        cond = float(np.linalg.cond(A1f))
        trail = 2 * m * mpmath.fsum(abs(u[i]) * av[i] for i in range(p)) / R
        if reml:
            MI = Inv * A2 * Inv
            dT += mpmath.fsum(abs(Inv[i, j]) * aS2[i, j] + abs(MI[i, j]) * aS1[i, j] for i in range(p) for j in range(p))
            trail += mpmath.fsum(abs(Inv[i, j] * A2[i, j]) for i in range(p) for j in range(p))
        round_g = delta / 2 * (m * dQ / R + m * Q * dR / (R * R) + dT) + cond * delta / 2 * trail
        s1v = [mpmath.fsum(aS1[b, a] * av[a] for a in range(P)) for b in range(p)]
        round_gamma = mpmath.fsum(abs(Inv[p - 1, b]) * s1v[b] for b in range(p)) + cond * max(av[:p])
        ip = [abs(Inv[p - 1, b]) for b in range(p)]
        round_se = (dR / R + mpmath.fsum(ip[a] * aS1[a, b] * ip[b] for a in range(p) for b in range(p)) / ipp + cond) / 2
        round_ll = (m * dR / R + mpmath.fsum(abs(mpmath.log(x)) for x in w) + p * cond) / 2
        # the pivot margins of the fp64 rule
        Lf, ok = np.tril(A1f), True
        for j in range(p):
            if not Lf[j, j] > A1f[j, j] * PIVOT_CLEAR:
                ok = False
                break
            Lf[j:, j] /= math.sqrt(Lf[j, j])
            for k in range(j + 1, p):
                Lf[k:, k] -= Lf[k:, j] * Lf[k, j]
        ok = ok and float(R) > float(S1[p, p]) * PIVOT_CLEAR
        return {"theta": theta, "gamma": gamma, "se": se, "ll": ll / 2, "gp": abs(gp), "cond": cond, "round_g": round_g,
                "round_gamma": round_gamma, "round_se": round_se, "round_ll": round_ll, "pivots": ok}


def root(mk, theta0, reml, max_iter=200):
    """(code, theta, plain): the header's outline at 40 digits with the stop rule 1e-30; plain = every step was Newton's."""
    theta = mpmath.mpf(float(theta0))
    lo, hi, have_lo, have_hi, plain = mpmath.mpf(LLIM), mpmath.mpf(ULIM), False, False, True
    for _ in range(max_iter):
        e = mk.evaluate(theta, reml)
        if e is None:
            return 2, theta, False
        g, gp = e
        if g > 0:
            lo, have_lo = theta, True
        if g < 0:
            hi, have_hi = theta, True
        if g > 0 and theta >= ULIM:
            return 4, theta, False
        if g < 0 and theta <= LLIM:
            return 3, theta, False
        t = theta - g / gp if gp < 0 else None
        if t is None or not (lo < t < hi and abs(t - theta) <= STEP_MAX):
            plain = False
            if (g > 0 and have_hi) or (g < 0 and have_lo):
                t = (lo + hi) / 2
            elif g > 0:
                t = min(theta + STEP_MAX, mpmath.mpf(ULIM))
            elif g < 0:
                t = max(theta - STEP_MAX, mpmath.mpf(LLIM))
            else:
                t = theta
        if abs(t - theta) <= mpmath.mpf(10) ** -30:
            return 0, theta, plain
        theta = t
    return 1, theta, False


def marker_truth(lam, UtX, Uty, z, theta0, reml):
    """One marker -> {field: float}.  clear = 1: the path from theta0 is plain Newton to an interior root and the pivots keep their margin."""
    with mpmath.workdps(DPS):
        out = dict.fromkeys(FIELDS, float("nan"))
        out["clear"] = 0.0
        mk = _Marker(lam, UtX, Uty, z)
        code, theta, plain = root(mk, theta0, reml)
        out["code"] = float(code)
        if code == 2:
            return out
        a = mk.evaluate(theta, reml, full=True)
        hstep = mpmath.mpf(10) ** -12                                     # central differences at 40 digits: 24 digits of the derivative
        up, dn = mk.evaluate(theta + hstep, reml, full=True), mk.evaluate(theta - hstep, reml, full=True)
        out.update({k: float(a[k]) for k in FIELDS if k in a})
        out["d_gamma"] = float(abs(up["gamma"] - dn["gamma"]) / (2 * hstep))
        out["d_se"] = float(abs(up["se"] - dn["se"]) / (2 * hstep))
        out["clear"] = float(code == 0 and plain and a["pivots"] and LLIM + 1 < theta < ULIM - 1)
        return out


def bounds(n, tol, t, m=None):
    """(bound of |theta - theta*|, of |gamma - gamma*|, of |se - se*|, of |l - l*|) of a converged fit with stop rule `tol` over n
    eigen-directions, from the truth t (row m of a panel's truth).  theta: the stop rule -- Newton converges quadratically, the error
    left after a step <= tol is far below tol -- plus what the rounding of g moves its root by, eps round_g / |g'(theta*)|.  gamma and
    se are those of the last evaluation, at a theta within that bound: its distance times their derivative in theta, plus their own
    rounding.  l has the derivative g, which is zero at the root: |g' dtheta + eps round_g| dtheta, plus its own rounding."""
    g = (lambda k: t[k]) if m is None else (lambda k: t[k][m])
    eps = 8.0 * (n + 16) * U53
    dth = tol + eps * g("round_g") / g("gp")
    return (dth, dth * g("d_gamma") + eps * g("round_gamma"), dth * g("d_se") + eps * g("round_se") * g("se"),
            dth * (g("gp") * dth + eps * g("round_g")) + eps * g("round_ll"))


def _one(args):
    return marker_truth(*args)


def panel_truth(lam, UtX, Uty, Zrows, theta0, reml, procs=1):
    jobs = [(lam, UtX, Uty, Zrows[i], theta0, reml) for i in range(Zrows.shape[0])]
    if procs > 1:
        import multiprocessing
        with multiprocessing.Pool(procs) as pool:
            rows = pool.map(_one, jobs, chunksize=1)
    else:
        rows = [_one(j) for j in jobs]
    return {k: np.array([r[k] for r in rows], dtype=np.float64) for k in FIELDS}


# ------------------------------------------------------------------------------------------------ the panels
def shape(name):
    """(n, L, c) of a named panel: "n<n>" (L = 5, c = 2), "L<L>" (n = 67, c = 2), "c<c>" (n = 67, L = 5)."""
    kind, v = name[0], int(name[1:])
    return {"n": (v, 5, 2), "L": (67, v, 2), "c": (67, 5, v)}[kind]


def all_panels():
    return ["n%d" % v for v in NS] + ["L%d" % v for v in LS] + ["c%d" % v for v in CS]


def _polymorphic(n, rows, seed):
    """`rows` seeded random markers (int8 -1 / 0 / +1, marker-major) with at least four individuals off the commonest genotype."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < rows:
        f = 0.15 + 0.7 * rng.random()
        g = (rng.random(n) < f).astype(np.int8) + (rng.random(n) < f).astype(np.int8) - 1
        if n - np.bincount(g + 1, minlength=3).max() >= 4:
            out.append(g)
    return np.array(out, dtype=np.int8)


def panel(name, seed=None):
    """(G (max(LK, L), n) int8 markers: K is made of the first LK = max(0.4 n, 4) -- a kinship of low rank plus 0.95 I, whose two groups
    of eigenvalues make delta identifiable at these small n --, Mt8 = G[:L]: the tested ones, X (n, c), y (n), LK) of a named panel.
    Only integers and elementwise fp64 operations: the same bits on every machine."""
    n, L, c = shape(name)
    seed = SEEDS[name] if seed is None else seed
    LK = max(int(0.4 * n), 4)
    G = _polymorphic(n, max(LK, L), seed)
    rng = np.random.default_rng(seed + 1)
    X = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])
    eff = rng.integers(-1, 2, size=LK)                                    # integer marker effects: the polygenic part, exact
    poly = (G[:LK].astype(np.int64).T @ eff).astype(np.float64) * (1.5 / math.sqrt(LK))
    y = 1.35 * rng.standard_normal(n) + poly + 0.5 * G[0].astype(np.float64)   # marker 0 is planted
    for j in range(c):
        y = y + X[:, j] * (0.3 if j % 2 == 0 else -0.2)
    return G, np.ascontiguousarray(G[:L]), X, y, LK


def kinship(G):
    """K = G' G / max + 0.95 I as calcMMt forms it (the product is of integers: exact)."""
    Gi = G.astype(np.int64)
    MMt = (Gi.T @ Gi).astype(np.float64)
    return MMt / MMt.max() + 0.95 * np.eye(G.shape[1])


def operands(name, seed=None):
    """What the rule takes, made on THIS machine: (lam, U, UtX, Uty, Zrows, theta0 REML, theta0 ML, Mt8, X, y)."""
    from eagleeverything_amd import am
    G, Mt8, X, y, LK = panel(name, seed)
    lam, U = np.linalg.eigh(kinship(G[:LK]))
    UtX, Uty = U.T @ X, U.T @ y
    th = [min(max(math.log(f(lam, UtX, Uty)["delta"]), -10.0), 10.0) for f in (am.emma_REMLE_eig, am.emma_MLE_eig)]
    return lam, U, UtX, Uty, Mt8.astype(np.float64) @ U, th[0], th[1], Mt8, X, y


def special(kind, n=67, seed=77):
    """Panels whose outcome is a code, not a root -> (lam, U, X, y, Mt8, the rows that must get the code, the code).
    "singular": row 0 monomorphic, row 1 equal to X's second column -> 2.  "upper": the trait's variance lies where K weighs least
    (no polygenic part: every marker's optimum is at theta = +10) -> 4.  "lower": it lies along K's leading direction with almost no
    noise -> 3."""
    G = _polymorphic(n, 2 * n, seed)
    lam, U = np.linalg.eigh(kinship(G))
    rng = np.random.default_rng(seed + 1)
    Mt8 = np.ascontiguousarray(G[:6]).copy()
    X = np.column_stack([np.ones(n), rng.standard_normal(n)])
    if kind == "singular":
        Mt8[0] = 1
        X[:, 1] = Mt8[1]
        return lam, U, X, 0.5 * rng.standard_normal(n) + 0.5 * G[3], Mt8, [0, 1], 2
    k = 0 if kind == "upper" else n - 1
    y = X @ np.array([0.3, -0.2]) + 3.0 * U[:, k] + 1e-3 * rng.standard_normal(n)
    return lam, U, X, y, Mt8, list(range(6)), 4 if kind == "upper" else 3


def digest(G, X, y):
    h = hashlib.sha256()
    for a in (np.ascontiguousarray(G, dtype=np.int8), np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)):
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


_cache = {}


def golden(name):
    """{"reml": truth, "ml": truth} of a named panel from tests/golden/lmm_truth.npz, after its digest is checked."""
    if "npz" not in _cache:
        _cache["npz"] = dict(np.load(GOLDEN))
    z = _cache["npz"]
    G, _, X, y, _ = panel(name)
    assert str(z[name + "/digest"]) == digest(G, X, y), "tests/golden/lmm_truth.npz was made from other inputs: " + name
    return {m: {k: z["%s/%s/%s" % (name, m, k)] for k in FIELDS} for m in ("reml", "ml")}


def _clear_share(args):
    name, seed = args
    lam, U, UtX, Uty, Zrows, th_r, th_m, _, _, _ = operands(name, seed)
    worst = 1.0
    for reml, th in ((True, th_r), (False, th_m)):
        worst = min(worst, float(panel_truth(lam, UtX, Uty, Zrows, th, reml)["clear"].mean()))
    return worst


def seed_search(procs=8, tries=160):
    """The SEEDS table: per panel the first of base, base + 1000, ... with at least 90 % clear markers under both methods."""
    import multiprocessing
    out = {}
    with multiprocessing.Pool(procs) as pool:
        for name in all_panels():
            base = {"n": 11000, "L": 12000, "c": 13000}[name[0]] + int(name[1:])
            for k0 in range(0, tries, procs):
                sh = pool.map(_clear_share, [(name, base + 1000 * k) for k in range(k0, k0 + procs)])
                hit = [k0 + i for i, v in enumerate(sh) if v >= 0.9]
                if hit:
                    out[name] = base + 1000 * hit[0]
                    break
            print(name, out.get(name), flush=True)
    return out


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["seeds"]:
        print(seed_search(int(os.environ.get("TRUTH_PROCS", "8"))))
        sys.exit(0)
    out = {}
    for name in all_panels():
        lam, U, UtX, Uty, Zrows, th_r, th_m, Mt8, X, y = operands(name)
        out[name + "/digest"] = np.array(digest(panel(name)[0], X, y))
        for m, th in (("reml", th_r), ("ml", th_m)):
            t = panel_truth(lam, UtX, Uty, Zrows, th, m == "reml", procs=int(os.environ.get("TRUTH_PROCS", "8")))
            for k, v in t.items():
                out["%s/%s/%s" % (name, m, k)] = v
            print(name, m, "theta0 %.3f  clear %d of %d  codes %s  max cond %.2g" % (th, t["clear"].sum(), len(t["clear"]),
                  sorted(set(t["code"].astype(int))), np.nanmax(t["cond"])), flush=True)
    np.savez_compressed(GOLDEN, **out)
