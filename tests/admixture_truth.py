"""Truth for the admixture EM step of include/eagle_hip.h section 1b''''v, in mpmath at 40 digits: one step (Q, F) -> (Q', F') and the
log-likelihood l(Q, F), written here from the rule alone -- nothing is shared with r_api.admixture_host or the kernels but the rule --
with the planted panels and inputs of tests/test_admixture_host.py and tests/test_gpu_admixture.py and the rounding bounds both hold.

Rounding bounds (u = 2^-53).  Every sum of the rule has non-negative terms, so a sum of N terms that each carry a relative error e is
off by at most (N + e / u) u relative, in any order.  p and pbar are sums of K products (K + 1 roundings); A and B add a division; a
sum over n individuals (sa, sb: n terms) or over the markers (t: 2 L terms) adds its length; the closing products, the quotient, the
floor and the normalisation over K add a handful more: at most (2 max(n, L) + K + 8) u per sum.  f' and q' are quotients of two such
sums, which doubles it to (4 max(n, L) + 2 K + 16) u, and the bound leaves a factor of two on top:
    each f', q':   relative error <= 8 (max(n, L) + K + 16) u, and
    l:             absolute error <= 2 n L (K + 4) u + n L u |l|:
each of the 2 n L terms d ln p carries the (K + 1) u relative error of p as an absolute error of at most 2 (K + 1) u plus the rounding
of ln and of the product, and the sum of the n L terms adds its length relative to sum |term| = |l| (all terms are <= 0)."""
import itertools

import mpmath
import numpy as np

DPS = 40
EPS = 1e-6
U = 2.0 ** -53

HOST_SHAPES = [(17, 16), (33, 50)]                      # one step against mpmath
HOST_KS = [1, 2, 5]
EM_PANELS = [(120, 600, 3), (33, 50, 2), (17, 16, 1), (64, 257, 5)]     # (n, L, K): 300 host steps


def rel_bound(n, L, K):
    return 8.0 * (max(n, L) + K + 16) * U


def ll_bound(n, L, K, ll):
    return 2.0 * n * L * (K + 4) * U + n * L * U * abs(ll)


def planted_panel(n, L, K, seed):
    """(Mt8 int8 (L, n), Q (n, K), F (L, K)): Q one Dirichlet(0.3) draw per individual, F from Beta(1/2, 1/2) clipped to [0.02, 0.98],
    genotypes Binomial(2, p); the marker rows 0, 1, 2 are all-0, all-2 and all-1 copies."""
    rng = np.random.default_rng(seed)
    Q = rng.dirichlet(np.full(K, 0.3), size=n)
    F = np.clip(rng.beta(0.5, 0.5, size=(L, K)), 0.02, 0.98)
    Mt8 = (rng.binomial(2, Q @ F.T).T - 1).astype(np.int8)
    for r, v in enumerate((-1, 1, 0)):
        if r < L:
            Mt8[r] = v
    return Mt8, Q, F


def marker_freq(Mt8):
    return (np.asarray(Mt8, dtype=np.float64) + 1.0).mean(axis=1) / 2.0


def planted_inputs(n, L, K, seed):
    """(Q (n, K), F (L, K)) that eagle_admixture_em accepts, with planted extremes: f at eps and at 1 - eps; q at 0 (row i = 3 mod 7
    loses its first component, individual 0 its last: with n = 1 that population has no individual at all) and at 1 (a unit vector on
    either side of every multiple of 16, on different components)."""
    rng = np.random.default_rng(seed)
    Q = rng.dirichlet(np.ones(K), size=n)
    F = rng.uniform(0.05, 0.95, size=(L, K))
    mk = np.add.outer(np.arange(L), np.arange(K))
    F[mk % 11 == 0] = EPS
    F[mk % 13 == 5] = 1.0 - EPS
    if K >= 2:
        Q[3::7, 0] = 0.0
        Q[0, K - 1] = 0.0
        for b in range(16, n, 16):
            Q[b - 1], Q[b] = 0.0, 0.0
            Q[b - 1, (b // 16) % K], Q[b, (b // 16 + 1) % K] = 1.0, 1.0
    Q = Q / Q.sum(axis=1, keepdims=True)
    return Q, F


def mp_step(Mt8, Q, F):
    """(Q', F', l(Q, F)) at 40 digits from the fp64 inputs taken exactly; Q', F' rounded to fp64 at the very end."""
    mpmath.mp.dps = DPS
    mpf = mpmath.mpf
    G = np.asarray(Mt8)
    L, n = G.shape
    K = Q.shape[1]
    q = [[mpf(float(Q[i, k])) for k in range(K)] for i in range(n)]
    f = [[mpf(float(F[m, k])) for k in range(K)] for m in range(L)]
    eps = mpf(EPS)
    ll = mpf(0)
    sa = [[mpf(0)] * K for _ in range(L)]
    sb = [[mpf(0)] * K for _ in range(L)]
    t = [[mpf(0)] * K for _ in range(n)]
    for m in range(L):
        for i in range(n):
            d = int(G[m, i]) + 1
            p = sum(q[i][k] * f[m][k] for k in range(K))
            pb = sum(q[i][k] * (1 - f[m][k]) for k in range(K))
            if d:
                ll += d * mpmath.log(p)
            if d != 2:
                ll += (2 - d) * mpmath.log(pb)
            A, B = d / p, (2 - d) / pb
            for k in range(K):
                sa[m][k] += q[i][k] * A
                sb[m][k] += q[i][k] * B
                t[i][k] += f[m][k] * A + (1 - f[m][k]) * B
    Fn = np.zeros((L, K))
    for m in range(L):
        for k in range(K):
            a, b = f[m][k] * sa[m][k], (1 - f[m][k]) * sb[m][k]
            v = a / (a + b) if a + b > 0 else f[m][k]
            Fn[m, k] = float(min(max(v, eps), 1 - eps))
    Qn = np.zeros((n, K))
    for i in range(n):
        row = [max(q[i][k] * t[i][k] / (2 * L), eps) for k in range(K)]
        s = sum(row)
        for k in range(K):
            Qn[i, k] = float(row[k] / s)
    return Qn, Fn, float(ll)


def assert_close(got, want, n, L, K, what=""):
    """got = (Q', F', l before[, l after]) against want within the bounds above; prints each figure before it asserts."""
    rb = rel_bound(n, L, K)
    eq = float(np.max(np.abs(got[0] - want[0]) / want[0]))
    ef = float(np.max(np.abs(got[1] - want[1]) / want[1]))
    print("%s n=%d L=%d K=%d: rel q' %.3g  rel f' %.3g  (bound %.3g)" % (what, n, L, K, eq, ef, rb))
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert eq <= rb and ef <= rb, (what, n, L, K, eq, ef, rb)
    for a, b in zip(got[2:], want[2:]):
        lb = ll_bound(n, L, K, b)
        print("    l %.17g against %.17g (bound %.3g)" % (a, b, lb))
        assert abs(a - b) <= lb, (what, n, L, K, a, b, lb)


def best_permutation_corr(Q, Qtrue):
    """The mean column correlation of Q with Qtrue under the best assignment of columns."""
    K = Q.shape[1]
    C = np.corrcoef(Q.T, Qtrue.T)[:K, K:]
    return max(float(np.mean([C[p[k], k] for k in range(K)])) for p in itertools.permutations(range(K)))
