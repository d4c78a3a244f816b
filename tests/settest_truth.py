"""Truth for the set statistics of include/eagle_hip.h section 1d'', in mpmath at 40 digits: per set the augmented weighted Gram, the
Schur complement on the U^T X block (scores s, covariance Phi), the degenerate-marker rule and the seven statistics (Q, Ub, Vb, c_1 ..
c_4), written here from the rule alone -- nothing is shared with r_api.settest_host or the kernel but the rule -- and first-order bounds
of what fp64 rounding does to each of them (below).

The panels are those of tests/lmm_truth.py (panel(), kinship(): a seeded genotype matrix G, K = G G' / max + 0.95 I of its first LK
rows, X, y; integers and elementwise fp64 operations only, so every machine makes the same bits): "n<n>" sweeps the eigen-directions over
the wave chunk at 64 and the four-wave round at 256, "m<m>" (lmm_truth's "L<m>" panel: n = 67, c = 2) the markers of a set over every
tile count and its edges, "c<c>" the columns of X; "x257" crosses them (n = 257, m = 64, c = 14: four marker tiles with all four waves live and a
second chunk in wave 0, made by lmm_truth's recipe at a shape it does not name); "deg" plants a monomorphic marker and one equal to a
column of X.  The markers of a panel are the first M rows of G (M = m for the m sweep and x257, min(rows, 20) otherwise); its sets (sets()) are all M markers with weights that
include a zero and are spread over 2^20, the first half in reversed order with weights 1, and marker 0 alone.  The variance components
are the same dyadic constants everywhere (VAR_E, VAR_G): the statistics are defined for any, and a fitted pair would differ in its
last bits from machine to machine.  lam, U = eigh(K) do differ so; the truth depends on K, X, y and the markers alone, not on the basis,
and what a basis rounded differently does enters like the rounding of the sums the bounds already carry (as in lmm_truth).

The truth costs a minute of mpmath, so it is computed once (`python tests/settest_truth.py` rewrites tests/golden/settest_truth.npz)
and keyed by a digest of each panel's inputs; tests/test_settest_host.py recomputes entries live.

Rounding bounds, to first order.  eps = 8 (n + 16) 2^-53 (the project's constant: a term of a Gram entry carries the roundings of d_k,
two products and its place in a sum of n) and u = 2^-53.  With E = |A|' diag(d) |A| the entrywise bound of the Gram's error per unit eps,
B = G_xx^-1 [G_xz | G_xy] with columns B_j (marker j) and B_y, and kappa = cond(G_xx) standing for the Cholesky solves (whose error is
a few c u kappa relative):
    d s_j    = eps varG   [E_zy[j] + E_zx[j] |B_y| + |B_j|' E_xy + |B_j|' E_xx |B_y| + kappa |G_zx[j]| |B_y|]
    d Phi_ij = eps varG^2 [E_zz[ij] + E_zx[i] |B_j| + |B_i|' E_xz[j] + |B_i|' E_xx |B_j| + kappa |G_zx[i]| |B_j|]
(the Schur complement is linear in dG_zz, dG_zx, dG_zy and carries dB = G_xx^-1 (dG_x. - dG_xx B) through G_zx G_xx^-1 = B').  With
Aw = W Phi W, dAw_ij = omega_i omega_j d Phi_ij + 3 u |Aw_ij|, |Aw| the entrywise absolute value and F the Frobenius norm:
    d Q   = 2 sum_j omega_j^2 |s_j| d s_j + (m + 2) u Q              d Ub = sum_j omega_j d s_j + (m + 1) u sum_j |omega_j s_j|
    d Vb  = sum_ij dAw_ij + m^2 u sum_ij |Aw_ij|                     d c_1 = sum_i dAw_ii + m u sum_i |Aw_ii|
    d c_r = r |Aw|_F^(r-1) |dAw|_F + (m^2 + r m + 2) u tr(|Aw|^r)    (r = 2, 3, 4: the first term is |d tr(Aw^r)| <= r |Aw^(r-1)|_F
                                                                     |dAw|_F, the second the m u per product and the final sum)
A marker the rule calls degenerate has s_j = 0 and its row and column of Phi exactly 0: no bound is needed there, and none is spent."""
import hashlib
import math
import os

import mpmath
import numpy as np

import lmm_truth as LT

DPS = 40
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "settest_truth.npz")
NS = [20, 63, 64, 65, 255, 256, 257, 1003]
MS = [1, 2, 15, 16, 17, 33, 48, 49, 64]
CS = [1, 2, 14]
VAR_E, VAR_G = 1.25, 0.75
PIVOT_REL = 2.0 ** -40
PIVOT_CLEAR = 2.0 ** -30      # a clear marker keeps a margin of 2^10 over the degenerate threshold
U53 = 2.0 ** -53
# One seed per panel, chosen (`python tests/settest_truth.py seeds`) as the first of base, base + 1000, ... for which every marker that is
# not planted is clear; tests/test_settest_host.py asserts that they are.
SEEDS = {"n20": 31020, "n63": 31063, "n64": 31064, "n65": 31065, "n255": 31255, "n256": 31256, "n257": 31257, "n1003": 32003,
         "m1": 33001, "m2": 33002, "m15": 33015, "m16": 33016, "m17": 33017, "m33": 33033, "m48": 33048, "m49": 33049, "m64": 33064,
         "c1": 34001, "c2": 34002, "c14": 34014, "x257": 36257, "deg": 35000}
STATS = ("Q", "Ub", "Vb", "c1", "c2", "c3", "c4")


def all_panels():
    return ["n%d" % v for v in NS] + ["m%d" % v for v in MS] + ["c%d" % v for v in CS] + ["x257", "deg"]


def small_panels():
    return ["n20", "m2", "m17", "c14", "deg"]


def panel(name, seed=None):
    """(G, Mt8 (M, n) int8: the markers, X (n, c), y (n), LK) of a named panel, from lmm_truth.panel."""
    seed = SEEDS[name] if seed is None else seed
    if name == "deg":
        G, _, X, y, LK = LT.panel("c2", seed)
        G = G.copy()
        G[0] = 1                                                            # monomorphic: in the span of the intercept
        X = X.copy()
        X[:, 1] = G[1]                                                      # marker 1 is a column of X
        return G, np.ascontiguousarray(G[:10]), X, y, LK
    if name == "x257":
        G, X, y, LK = _cross_panel(257, 64, 14, seed)
        return G, np.ascontiguousarray(G[:64]), X, y, LK
    G, _, X, y, LK = LT.panel(("L" + name[1:]) if name[0] == "m" else name, seed)
    M = int(name[1:]) if name[0] == "m" else min(G.shape[0], 20)
    return G, np.ascontiguousarray(G[:M]), X, y, LK


def _cross_panel(n, L, c, seed):
    """lmm_truth.panel's recipe (integers and elementwise fp64 operations only) at a shape its names do not reach -> (G, X, y, LK)."""
    LK = max(int(0.4 * n), 4)
    G = LT._polymorphic(n, max(LK, L), seed)
    rng = np.random.default_rng(seed + 1)
    X = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])
    eff = rng.integers(-1, 2, size=LK)
    poly = (G[:LK].astype(np.int64).T @ eff).astype(np.float64) * (1.5 / math.sqrt(LK))
    y = 1.35 * rng.standard_normal(n) + poly + 0.5 * G[0].astype(np.float64)
    for j in range(c):
        y = y + X[:, j] * (0.3 if j % 2 == 0 else -0.2)
    return G, X, y, LK


def weights(m):
    """m dyadic weights spread over 2^20, the second one zero (from m = 3 on)."""
    w = np.array([2.0 ** ((7 * j) % 21) for j in range(m)])
    if m >= 3:
        w[1] = 0.0
    return w


def sets(name, M):
    """(sets, omega) of a panel with M markers."""
    if name == "deg":
        return [np.arange(M), np.array([0, 1]), np.array([2])], [weights(M), np.ones(2), np.ones(1)]
    half = np.arange((M + 1) // 2)[::-1].copy()
    return [np.arange(M), half, np.array([0])], [weights(M), np.ones(half.size), np.ones(1)]


def operands(name, seed=None):
    """What the rule takes, made on THIS machine: (lam, U, UtX, Uty, Zrows (M, n), Mt8, X, y, sets, omega)."""
    G, Mt8, X, y, LK = panel(name, seed)
    lam, U = np.linalg.eigh(LT.kinship(G[:LK]))
    st, om = sets(name, Mt8.shape[0])
    return lam, U, U.T @ X, U.T @ y, Mt8.astype(np.float64) @ U, Mt8, X, y, st, om


def digest(G, X, y):
    return LT.digest(G, X, y)


# ------------------------------------------------------------------------------------------------ the rule in mpmath
def _mp(v):
    return mpmath.mpf(float(v))


def set_truth(lam, UtX, Uty, Zset, omega, varE=VAR_E, varG=VAR_G):
    """One set -> dict of float arrays: stat (7), s (m), Phi (m, m), deg (m), code, n_used, margin (the smallest Phi_jj / (varG^2
    G_zz,jj) over the markers that are not degenerate; inf without one), and the bounds b_stat (7), b_s (m), b_Phi (m, m)."""
    with mpmath.workdps(DPS):
        n = len(lam)
        Ut = np.asarray(UtX, dtype=np.float64).reshape(n, -1)
        A = np.column_stack([np.asarray(Zset, dtype=np.float64).reshape(-1, n).T, Ut, np.asarray(Uty, dtype=np.float64).ravel()])
        m, c = A.shape[1] - Ut.shape[1] - 1, Ut.shape[1]
        P = m + c + 1
        vE, vG = _mp(varE), _mp(varG)
        d = [1 / (vE + vG * _mp(l)) for l in lam]
        cols = [[_mp(v) for v in A[:, a]] for a in range(P)]
        G, E = mpmath.zeros(P), mpmath.zeros(P)
        for a in range(P):
            da = [x * w for x, w in zip(cols[a], d)]
            ada = [abs(x) for x in da]
            for b in range(a + 1):
                G[a, b] = G[b, a] = mpmath.fdot(da, cols[b])
                E[a, b] = E[b, a] = mpmath.fdot(ada, [abs(x) for x in cols[b]])
        X0, Y = m, m + c
        Gxx = G[X0:Y, X0:Y]
        Inv = Gxx ** -1
        rhs = mpmath.zeros(c, m + 1)
        for a in range(c):
            for j in range(m):
                rhs[a, j] = G[X0 + a, j]
            rhs[a, m] = G[X0 + a, Y]
        B = Inv * rhs
        aB = B.apply(abs)
        kappa = float(np.linalg.cond(np.array([[float(Gxx[i, j]) for j in range(c)] for i in range(c)])))
        s = [vG * (G[j, Y] - mpmath.fsum(G[j, X0 + a] * B[a, m] for a in range(c))) for j in range(m)]
        Phi = mpmath.zeros(m)
        for i in range(m):
            for j in range(i + 1):
                Phi[i, j] = Phi[j, i] = vG * vG * (G[i, j] - mpmath.fsum(G[i, X0 + a] * B[a, j] for a in range(c)))
        # rounding per unit eps
        ExB = [[mpmath.fsum(E[X0 + a, X0 + b] * aB[b, j] for b in range(c)) for j in range(m + 1)] for a in range(c)]     # E_xx |B_j|

        def cross(i, j, gj):
            """E[i, gj] + E_zx[i] |B_j| + |B_i|' E_x,gj + |B_i|' E_xx |B_j| + kappa |G_zx[i]| |B_j| (j = m, gj = Y: the y column)."""
            return (E[i, gj] + mpmath.fsum(E[i, X0 + a] * aB[a, j] for a in range(c)) + mpmath.fsum(aB[a, i] * E[X0 + a, gj] for a in range(c))
                    + mpmath.fsum(aB[a, i] * ExB[a][j] for a in range(c)) + kappa * mpmath.fsum(abs(G[i, X0 + a]) * aB[a, j] for a in range(c)))

        r_s = [vG * cross(j, m, Y) for j in range(m)]
        r_Phi = mpmath.zeros(m)
        for i in range(m):
            for j in range(i + 1):
                r_Phi[i, j] = r_Phi[j, i] = vG * vG * cross(i, j, j)
        # the degenerate-marker rule
        ratio = [Phi[j, j] / (vG * vG * G[j, j]) if G[j, j] > 0 else mpmath.mpf(0) for j in range(m)]
        deg = [not (ratio[j] > PIVOT_REL) for j in range(m)]
        live = [float(ratio[j]) for j in range(m) if not deg[j]]
        for j in range(m):
            if deg[j]:
                s[j] = r_s[j] = mpmath.mpf(0)
                for i in range(m):
                    Phi[i, j] = Phi[j, i] = r_Phi[i, j] = r_Phi[j, i] = mpmath.mpf(0)
        om = [_mp(w) for w in omega]
        eps, u = 8.0 * (n + 16) * U53, U53
        Aw, dAw = mpmath.zeros(m), mpmath.zeros(m)
        for i in range(m):
            for j in range(m):
                Aw[i, j] = om[i] * Phi[i, j] * om[j]
                dAw[i, j] = eps * om[i] * om[j] * r_Phi[i, j] + 3 * u * abs(Aw[i, j])
        aAw = Aw.apply(abs)
        Aw2, aAw2 = Aw * Aw, aAw * aAw
        fro = lambda Mx: mpmath.sqrt(mpmath.fsum(Mx[i, j] ** 2 for i in range(m) for j in range(m)))
        had = lambda Mx, My: mpmath.fsum(Mx[i, j] * My[i, j] for i in range(m) for j in range(m))
        t = [om[j] * s[j] for j in range(m)]
        Q, Ub = mpmath.fsum(x * x for x in t), mpmath.fsum(t)
        Vb, c1 = mpmath.fsum(Aw[i, j] for i in range(m) for j in range(m)), mpmath.fsum(Aw[i, i] for i in range(m))
        c2, c3, c4 = had(Aw, Aw), had(Aw, Aw2), had(Aw2, Aw2)
        nA, nd = fro(Aw), fro(dAw)
        b_stat = [2 * eps * mpmath.fsum(om[j] ** 2 * abs(s[j]) * r_s[j] for j in range(m)) + (m + 2) * u * Q,
                  eps * mpmath.fsum(om[j] * r_s[j] for j in range(m)) + (m + 1) * u * mpmath.fsum(abs(x) for x in t),
                  mpmath.fsum(dAw[i, j] for i in range(m) for j in range(m)) + m * m * u * mpmath.fsum(aAw[i, j] for i in range(m) for j in range(m)),
                  mpmath.fsum(dAw[i, i] for i in range(m)) + m * u * mpmath.fsum(aAw[i, i] for i in range(m)),
                  2 * nA * nd + (m * m + 2 * m + 2) * u * had(aAw, aAw),
                  3 * nA ** 2 * nd + (m * m + 3 * m + 2) * u * had(aAw, aAw2),
                  4 * nA ** 3 * nd + (m * m + 4 * m + 2) * u * had(aAw2, aAw2)]
        none = not (Vb > 0) or not (c2 > 0)
        f = lambda Mx: np.array([[float(Mx[i, j]) for j in range(m)] for i in range(m)])
        return {"stat": np.array([float(v) for v in (Q, Ub, Vb, c1, c2, c3, c4)]), "s": np.array([float(v) for v in s]), "Phi": f(Phi),
                "deg": np.array(deg, dtype=np.float64), "code": np.array(2.0 if none else 0.0), "n_used": np.array(float(m - sum(deg))),
                "margin": np.array(min(live) if live else float("inf")), "kappa": np.array(kappa),
                "b_stat": np.array([float(v) for v in b_stat]), "b_s": np.array([eps * float(v) for v in r_s]), "b_Phi": eps * f(r_Phi)}


FIELDS = ("stat", "s", "Phi", "deg", "code", "n_used", "margin", "kappa", "b_stat", "b_s", "b_Phi")


def panel_truth(name, seed=None):
    """[set_truth of every set of the panel], from this machine's operands."""
    lam, U, UtX, Uty, Z, Mt8, X, y, st, om = operands(name, seed)
    return [set_truth(lam, UtX, Uty, Z[j], w) for j, w in zip(st, om)]


_cache = {}


def golden(name):
    """[truth of every set] of a named panel from tests/golden/settest_truth.npz, after its digest is checked."""
    if "npz" not in _cache:
        _cache["npz"] = dict(np.load(GOLDEN))
    z = _cache["npz"]
    G, _, X, y, _ = panel(name)
    assert str(z[name + "/digest"]) == digest(G, X, y), "tests/golden/settest_truth.npz was made from other inputs: " + name
    return [{k: z["%s/%d/%s" % (name, o, k)] for k in FIELDS} for o in range(int(z[name + "/nsets"]))]


def planted(name, o):
    """The markers of set o of a panel that are planted degenerate (positions in the set)."""
    return {0: [0, 1], 1: [0, 1], 2: []}[o] if name == "deg" else []


def is_clear(name, truth):
    """The seed condition: every marker that is not planted keeps a margin of 2^10 over the degenerate threshold, and the planted
    ones are degenerate."""
    for o, t in enumerate(truth):
        pl = planted(name, o)
        if [j for j in np.flatnonzero(t["deg"] > 0.5)] != pl or not float(t["margin"]) > PIVOT_CLEAR:
            return False
    return True


def _clear(args):
    name, seed = args
    return is_clear(name, panel_truth(name, seed))


def seed_search(procs=8, tries=64):
    import multiprocessing
    out = {}
    with multiprocessing.Pool(procs) as pool:
        for name in all_panels():
            base = SEEDS[name]
            for k0 in range(0, tries, procs):
                ok = pool.map(_clear, [(name, base + 1000 * k) for k in range(k0, k0 + procs)])
                hit = [k0 + i for i, v in enumerate(ok) if v]
                if hit:
                    out[name] = base + 1000 * hit[0]
                    break
            print(name, out.get(name), flush=True)
    return out


def _panel_entries(name):
    G, _, X, y, _ = panel(name)
    out = {name + "/digest": np.array(digest(G, X, y))}
    truth = panel_truth(name)
    out[name + "/nsets"] = np.array(len(truth))
    for o, t in enumerate(truth):
        for k in FIELDS:
            out["%s/%d/%s" % (name, o, k)] = t[k]
    return name, out, is_clear(name, truth), max(float(t["kappa"]) for t in truth)


if __name__ == "__main__":
    import multiprocessing
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    procs = int(os.environ.get("TRUTH_PROCS", "8"))
    if sys.argv[1:] == ["seeds"]:
        print(seed_search(procs))
        sys.exit(0)
    out = {}
    with multiprocessing.Pool(procs) as pool:
        for name, ent, clear, kappa in pool.imap(_panel_entries, all_panels()):
            out.update(ent)
            print(name, "clear" if clear else "NOT CLEAR", "cond(G_xx) %.3g" % kappa, flush=True)
    np.savez_compressed(GOLDEN, **out)
