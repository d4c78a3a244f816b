"""Truth for the max(T) permutation pass (include/eagle_hip.h section 1b''''vi) by plain loops over individuals on Python ints and
Fractions: no numpy arithmetic, no matrix product, no vectorised hash.  tests/test_maxt_host.py pins r_api.maxt_host and
r_api.maxt_permutations_host to it; the GPU tests then hold the device to maxt_host with ==."""
from fractions import Fraction

MASK = (1 << 64) - 1
# the first outputs of splitmix64 from state 0 (Vigna's reference generator, the published seeding vectors of xoshiro256): the words
# the mixer must give for seed = 0 and counter = r 2^16 + j + 1 = 1, 2, 3, 4
SPLITMIX64_FROM_ZERO = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC]


def mix64(seed, r, j):
    z = (seed + ((r << 16) + j + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def key64(seed, r, j, stratum):
    return (stratum << 48) | ((mix64(seed, r, j) >> 32) << 16) | j


def permutation(N, strata_used, seed, r):
    """Row r in the explicit form: t'[u_k] = t[u_row[k]]."""
    st = [0] * N if strata_used is None else [int(s) for s in strata_used]
    sigma = sorted(range(N), key=lambda j: (st[j], j))
    pi = sorted(range(N), key=lambda j: key64(seed, r, j, st[j]))
    row = [0] * N
    for k in range(N):
        row[sigma[k]] = pi[k]
    return row


def digits(t):
    m, sg = abs(t), (t > 0) - (t < 0)
    return [sg * (m & 127), sg * ((m >> 7) & 127), sg * ((m >> 14) & 127)]


def planes(tmax):
    return 1 if tmax <= 127 else (2 if tmax <= 16383 else 3)


def key_of(d, V):
    """fl(fl(d d) / V): float() of a Python int and the division of two floats are each correctly rounded."""
    return 0.0 if V == 0 else float(d * d) / float(V)


def maxt(Mt, t, used, strata, seed, first, R, perm=None):
    """Mt: L rows of n values in -1 / 0 / +1; t: n ints -> dict of lists, as eagle_maxt defines its outputs; "exact": key as a Fraction."""
    L, n = len(Mt), len(t)
    u = [i for i in range(n) if used is None or used[i]]
    N = len(u)
    T = sum(int(t[i]) for i in u)
    su = None if strata is None else [int(strata[i]) for i in u]
    S, V = [], []
    for m in range(L):
        s = q = 0
        for i in u:
            s += int(Mt[m][i])
            q += int(Mt[m][i]) ** 2
        S.append(s)
        V.append(N * q - s * s)

    def dvec(tp):
        out = []
        for m in range(L):
            c = 0
            for k, i in enumerate(u):
                c += int(Mt[m][i]) * tp[k]
            out.append(N * c - S[m] * T)
        return out

    tu = [int(t[i]) for i in u]
    d_obs = dvec(tu)
    count1, maxkey, argmax = [0] * L, [], []
    for q in range(R):
        row = [int(v) for v in perm[q]] if perm is not None else permutation(N, su, seed, first + q)
        assert sorted(row) == list(range(N))
        d = dvec([tu[row[k]] for k in range(N)])
        keys = [key_of(d[m], V[m]) for m in range(L)]
        for m in range(L):
            count1[m] += abs(d[m]) >= abs(d_obs[m])
        best = max(keys)
        maxkey.append(best)
        argmax.append(keys.index(best))
    return {"d_obs": d_obs, "V": V, "key_obs": [key_of(d_obs[m], V[m]) for m in range(L)], "count1": count1, "maxkey": maxkey,
            "argmax": argmax, "exact": [Fraction(d_obs[m] ** 2, V[m]) if V[m] else Fraction(0) for m in range(L)], "S": S, "N": N, "T": T}
