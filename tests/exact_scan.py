"""Operands of the marker scan whose true a and vara are integers (times a power of two), and that truth restated without the library
(not a conftest; shared by tests/test_scan_exact_host.py, which pins it on the CPU, and tests/test_gpu_scan_exact.py).

    S = s I (s = 1 or 2)        ->  W = S (V S) = s^2 V and v = S a_hat = s a_hat, no rounding in any product
    V = u X, X symmetric int64  ->  every W_jk is a multiple of u = 2^log2u; the diagonal is an integer above its row's |.| sum
    a_hat integer, |a_hat| <= 8

    a_i = sum_j m_ij v_j,     vara_i = sum_j W_jj m_ij^2 + 2 sum_{j<k} W_jk m_ij m_ik        (scan_truth)

Every partial sum any kernel can form is a sum of a subset of the terms m_j m_k Wu_jk of a (re-centred) marker, |m'| <= 2, or of the
digit parts of those terms (a balanced base-256 digit times its weight is at most 2.01 x the entry it was cut from).  check_exact()
bounds all of them by A = 4 s^2 (2 sum_{j<k} 2 |V_jk| + sum_j V_jj) in Python ints and demands A / u < 2^51 (a factor 4 of room for the
digit parts): below 2^53 units of u every such sum is a double, whatever the order.  fp64 has 53 bits, so the span between the largest
entry (2^22 - 1, which fixes the library's scale exponent e = 23 + 2 log2 s) and u is limited: the dense part of V is u x, |x| < 2^22 (the
three lowest digits of the slice count u stands for), and only as many entries of full height as the bound leaves room for."""
from fractions import Fraction

import numpy as np

MAXOFF = (1 << 22) - 1
EDGE_DIGITS = (-128, -127, -1, 0, 1, 127)
# u of the forced slice counts: unit of the last digit = 2^(e + 2 - 8 S) on the folded entries 2 W_jk, e = 23 -> u = 2^(24 - 8 S) puts x on the lowest
# digits.  S = 7 would need u = 2^-32, 55 bits below the largest entry: no double holds their sum.  2^-24 is the finest u of the 8-bit grid the
# exactness bound admits; there the patterns sit on digits 1..3 of 7 and digit 0 is zero.
LOG2U_OF_SLICES = {3: 0, 4: -8, 5: -16, 7: -24}


def edge_values():
    """d2 65536 + d1 256 + d0 over the edge digits and their negatives, inside +-(2^22 - 1), without 0: 214 values."""
    vals = set()
    for d2 in EDGE_DIGITS:
        for d1 in EDGE_DIGITS:
            for d0 in EDGE_DIGITS:
                x = d2 * 65536 + d1 * 256 + d0
                if x != 0 and abs(x) <= MAXOFF:
                    vals.update((x, -x))
    return sorted(vals)


def planted_pairs(n):
    """Where the edge values go: corners, both sides of every 256 / 384 boundary, inside one tile, across two tiles."""
    want = [(0, 1), (0, n - 1), (n - 2, n - 1), (255, 256), (383, 384), (511, 512), (767, 768), (3, 200), (130, 250), (100, 700), (260, 900), (381, 386)]
    out = []
    for j, k in want:
        if 0 <= j < k < n and (j, k) not in out:
            out.append((j, k))
    return out


def build_case(n, L, log2u=0, s=1, seed=0, small=False):
    """-> dict(Mt8 L x n int8, S, V, ahat, X int64 n x n (V / u), log2u, s, pairs, probes {pair: (row of e_j+e_k, e_j-e_k, e_j)}, zero, plus,
    minus, dup (first, second), max_pair).  small: |x| <= 3 everywhere (the operands of the int8 W engine's test), no planted values."""
    rng = np.random.default_rng(1000003 * n + 1009 * L + 17 * (-log2u) + s + 7919 * seed)
    sh = -log2u
    assert sh >= 0
    X = np.zeros((n, n), dtype=np.int64)
    iu = np.triu_indices(n, 1)
    npairs = iu[0].size
    pairs, max_pair = [], None
    if small:
        X[iu] = rng.integers(-3, 4, size=npairs)
    elif npairs:
        X[iu] = rng.integers(-MAXOFF, MAXOFF + 1, size=npairs)          # dense part: u x, the three lowest digits
        pairs = planted_pairs(n)
        cand = [(j, k) for j, k in ((n // 2, n // 2 + 1), (1, 2), (0, 1)) if 0 <= j < k < n and (n == 2 or (j, k) not in pairs)]
        max_pair = cand[0] if cand else pairs[0]
        if sh:   # entries of full height (every digit in use): as many as the exactness bound leaves room for (A ~ 24 s^2 sum_{j<k} |X_jk|)
            room = (1 << 51) // (24 * s * s) - npairs * (MAXOFF + 1) - ((MAXOFF + 1) << sh) - ((8 * n) << sh)
            K = int(max(0, min(npairs // 4, 4096, room // ((MAXOFF + 1) << sh) - 1)))
            pos = rng.choice(npairs, size=K, replace=False)
            X[iu[0][pos], iu[1][pos]] = rng.integers(-(MAXOFF << sh), (MAXOFF << sh) + 1, size=K)
        ev = edge_values()
        rng.shuffle(ev)
        scatter = rng.choice(npairs, size=min(npairs, len(ev)), replace=False)
        X[iu[0][scatter], iu[1][scatter]] = ev[:scatter.size]
        for t, (j, k) in enumerate(p for p in pairs if p != max_pair):
            X[j, k] = ev[t % len(ev)]
        pairs = [p for p in pairs if p != max_pair]
        X[max_pair] = MAXOFF << sh                                       # 2^22 - 1 in absolute value: e = 23 + 2 log2 s
    X = X + X.T
    rowabs = np.abs(X).sum(axis=1)
    D = -(-rowabs >> sh) + 1 + rng.integers(0, 5, size=n)              # integer, strictly above sum_k |V_jk|
    X[np.arange(n), np.arange(n)] = D << sh
    # markers: random genotypes (zero the commonest), then the probes and the special rows at the end of the panel
    Mt8 = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(L, n), p=[0.2, 0.55, 0.25])
    mstar = Mt8[0].copy()
    mstar[0] = 1
    if max_pair is not None and n >= 8:
        mstar[list(max_pair)] = 0                                       # keeps the largest W_jj out of its vara: marker 0 (and its duplicate) hold the largest tsq
    Mt8[0] = mstar
    out = dict(pairs=pairs, probes={}, zero=None, plus=None, minus=None, dup=None, max_pair=max_pair)
    special = 3 * len(pairs) + 4
    if L >= special + 8:
        r = L - special
        for (j, k) in pairs:
            for t, sk in enumerate((1, -1, 0)):
                Mt8[r + t] = 0
                Mt8[r + t, j] = 1
                Mt8[r + t, k] = sk
            out["probes"][(j, k)] = (r, r + 1, r + 2)
            r += 3
        Mt8[r] = 0
        Mt8[r + 1] = 1
        Mt8[r + 2] = -1
        Mt8[r + 3] = mstar                                              # the duplicate of marker 0, whose tsq a_hat = 8 m* makes the largest
        out.update(zero=r, plus=r + 1, minus=r + 2, dup=(0, r + 3))
    ahat = 8 * mstar.astype(np.int64)
    V = np.ldexp(X.astype(np.float64), log2u)
    assert np.array_equal(np.ldexp(V, sh).astype(np.int64), X)           # V = u X exactly
    out.update(Mt8=np.ascontiguousarray(Mt8), S=float(s) * np.eye(n), V=V, ahat=ahat.astype(np.float64), X=X, log2u=log2u, s=s, n=n, L=L)
    return out


def check_exact(case):
    """The bound of the module docstring, in Python ints: every partial sum of every evaluation order is a double.  Returns A / u."""
    X, s = case["X"], case["s"]
    n = X.shape[0]
    Xo = np.abs(X).astype(object)                                        # Python ints from here on
    rows = Xo.sum(axis=1) if n else []
    diag = sum(int(X[j, j]) for j in range(n))
    off2 = sum(int(r) for r in rows) - diag                              # sum_{j != k} |X_jk| = 2 sum_{j<k}
    assert all(int(X[j, j]) > int(rows[j]) - int(X[j, j]) for j in range(n)), "diagonal dominance"
    A = 4 * s * s * (2 * off2 + diag)
    assert A < (1 << 51), ("vara not exact in fp64 on these operands", A.bit_length())
    assert n <= 1003 and (8 * s * n) ** 2 < (1 << 53)                    # a^2
    offmax = max((int(x) for x in Xo[np.triu_indices(n, 1)]), default=0)
    assert offmax < ((1 << 22) << -case["log2u"])
    if case["max_pair"] is not None:
        assert offmax == int(X[case["max_pair"]]) == MAXOFF << -case["log2u"]
    return A


def _exact_matmul(M, Xf):
    """int64 M @ Xf for M in {-2..2} and int64 Xf through three 24-bit limbs, each an exact fp64 product (|sums| < 2^10 2 2^24)."""
    Mf = M.astype(np.float64)
    out = np.zeros((M.shape[0], Xf.shape[1]), dtype=np.int64)
    for limb in range(3):
        part = (Xf >> (24 * limb)) & 0xFFFFFF if limb < 2 else Xf >> 48   # the top limb carries the sign
        out += (Mf @ part.astype(np.float64)).astype(np.int64) << (24 * limb)
    return out


def fold_units(case):
    """Xf: W / (s^2 u) folded as the sum is written: W_jj on the diagonal, 2 W_jk above it, 0 below."""
    X = case["X"]
    return 2 * np.triu(X, 1) + np.diag(np.diag(X))


def scan_truth(case, Mt8=None):
    """-> (a, vara, vara in units of s^2 u as int64) of every marker, in int64: a_i = sum_j m_ij v_j,
    vara_i = sum_j W_jj m_ij^2 + 2 sum_{j<k} W_jk m_ij m_ik."""
    M = (case["Mt8"] if Mt8 is None else Mt8).astype(np.int64)
    s = case["s"]
    a = M @ (s * case["ahat"].astype(np.int64))
    units = (_exact_matmul(M, fold_units(case)) * M).sum(axis=1)
    assert np.abs(units).max(initial=0) < (1 << 53) and np.abs(a).max(initial=0) < (1 << 26)
    return a.astype(np.float64), np.ldexp(units.astype(np.float64), case["log2u"]) * (s * s), units


def scan_truth_fraction(case, rows):
    """The same two sums for the markers `rows` as a triple Python loop in Fraction."""
    X, s, u = case["X"], case["s"], Fraction(2) ** case["log2u"]
    n = X.shape[0]
    res = []
    for i in rows:
        m = [int(x) for x in case["Mt8"][i]]
        a = sum(Fraction(m[j]) * s * Fraction(int(case["ahat"][j])) for j in range(n))
        v = Fraction(0)
        for j in range(n):
            v += Fraction(int(X[j, j])) * u * s * s * m[j] * m[j]
            for k in range(j + 1, n):
                v += 2 * Fraction(int(X[j, k])) * u * s * s * m[j] * m[k]
        res.append((a, v))
    return res


def argmax_truth(a, units, case):
    """find_qtl.R:71-83 in rationals: (1-based first index of the largest a^2 / vara over the markers with vara != 0 or a != 0, that maximum as a
    Fraction), or (0, None) when every tsq is NaN (0 / 0)."""
    scale = Fraction(2) ** case["log2u"] * case["s"] ** 2
    best, idx = None, 0
    for i in range(len(a)):
        ai, vi = int(a[i]), int(units[i])
        if vi == 0:
            assert ai == 0, "a positive definite W has vara = 0 only for the zero marker"
            continue
        t = Fraction(ai * ai, 1) / (vi * scale)
        if best is None or t > best:
            best, idx = t, i + 1
    return idx, best


def digit_residual_units(case, S_cut, e):
    """r_jk / (s^2 u) above the diagonal for S_cut digits on the scale exponent e: folded entry minus unit * rint(entry / unit), unit =
    2^(e + 2 - 8 S_cut) (ties to even, as llrint)."""
    Xf = np.triu(fold_units(case), 1) * case["s"] ** 2                  # folded W in units of u
    sh = (e + 2 - 8 * S_cut) - case["log2u"]                             # log2(unit / u)
    if sh <= 0:
        return np.zeros_like(Xf)
    q = np.rint(np.ldexp(Xf.astype(np.float64), -sh)).astype(np.int64)   # |Xf| < 2^53: exact scaling, one correct rounding
    return Xf - (q << sh)


def ulp_distance(x, y):
    a, b = np.float64(x).view(np.int64), np.float64(y).view(np.int64)
    return abs(int(a) - int(b))
