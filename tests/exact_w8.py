"""Integer operands of W = S (V S) with a NON-diagonal S whose digit planes the int8 engine (csrc/eagle_w8.hip) holds exactly, and the
truth restated without the library (not a conftest; shared by tests/test_w8_exact_host.py, which pins it on the CPU, and
tests/test_gpu_w8_exact.py).  numpy and Python ints only.

k_w8_slice cuts row i of an image into six balanced base-256 planes of Q = llrint(M[i][l] 2^(46 - e_i)), e_i = w_scale_exp(max_l!=i
|M[i][l]|), plane 1 the most significant.  A row whose off-diagonal entries are multiples of 2^(e_i + 2 - 8 k) has planes k+1..6 empty and
is cut without rounding; a configuration (k, T) forms every plane pair p, q <= k, p + q <= T as exact int32 level sums.  So when no
non-empty pair lies outside the configuration that ran, G1, X = S V^T, G2 and W are exact and every summation order returns the same bits.

Two kinds (build_case), neither reaches every edge alone:
  "s1"  off-diagonal S on ONE plane: entries m 2^(e_i - 6), |m| <= 63, one entry 63 2^(e_i - 6) per row fixes e_i in {6, 7, 8} (pairs of
        rows share it); off-diagonal V on THREE planes: four `wide' rows c (two matched pairs) carry 100 2^16 + d2 256 + d3, which fixes
        their e = 22, and entries d2 256 + d3 with the edge digits {-128, -127, -1, 0, 1, 127}; the other rows a ring of d3 and entries d2 256 +
        d3 on both sides of every multiple of 128.  X then fits three planes per row: plane pairs (1, q <= 3) in both products.
  "s2"  off-diagonal S on TWO planes (e = 14, unit 1): entries d1 256 + d2 with the edge digits on plane 2 and values = 128 mod 256, which
        are cut as digit -128 with a carry into plane 1; one entry of about 2^14.2 per row fixes e.  V = I + a ring and scattered entries of
        +-1 (any |v| >= 2 next to the entry that fixes e would push X over 2^15 and onto a third plane), so X fits two planes: pairs <= (2, 2).
Why S is not full at large n, and why four rows carry a large diagonal: the engine accepts a W only when its rigorous bound -- which has a
floor of 2^-49 n times the operands' scales whatever the digits hold -- is below 2e-9 mean|W_kk|, and an exact truth needs every sum below
2^53 units of the last bit.  Both hold with about 32 off-diagonal entries per row of S (all of them up to n = 33) and wide rows with
S_cc = 2^12 (2^16), V_cc = 2^26 (2^18) and no off-diagonal S.  Those four rows of S are diagonal: rows without an exponent, a path of
k_w8_slice of its own.  Every product G1 = F Fv^T, G2 = F Fx^T still has non-zeros in every pair of 256- and 384-row tiles (asserted)."""
from fractions import Fraction

import numpy as np

KMAX = 6
EDGE_DIGITS = (-128, -127, -1, 0, 1, 127)
W8_CONFIGS = ((3, 4), (3, 5), (4, 5), (4, 6), (5, 6), (5, 7), (6, 7), (6, 8), (6, 9), (6, 12))
LIMIT = 1 << 53


def pad256(n):
    return (n + 255) // 256 * 256


def covered(pairs, k, T):
    """Every plane pair inside the configuration (k, T): p, q <= k, p + q <= T."""
    return all(p <= k and q <= k and p + q <= T for p, q in pairs)


def scale_exp(mx):
    """w_scale_exp of csrc/eagle_t8.h: mx = f 2^E, f in [0.5, 1); e = E, or E - 1 when f <= 0.98 (0 for an empty row)."""
    mx = np.asarray(mx, dtype=np.float64)
    f, E = np.frexp(mx)
    return np.where(mx > 0, np.where(f <= 0.98, E - 1, E), 0).astype(np.int64)


def planes(M, exact=True):
    """k_w8_slice restated from its header comment -> (e_i, digits[6][n][n] int64, plane 1 first); asserts that the planes reconstruct the
    off-diagonal part exactly: off(M)[i][l] = 2^(e_i + 2) sum_p 256^-p a_p[i][l].  exact=False: real-valued entries are rounded to the
    unit of plane 6 as llrint does (the one restatement of the slicer in the tests: tests/test_w8_host.py cuts with it too)."""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    F = M.copy()
    F[np.arange(n), np.arange(n)] = 0.0
    mx = np.abs(F).max(axis=1) if n else np.zeros(0)
    e = scale_exp(mx)
    scaled = np.ldexp(F, (8 * KMAX - e - 2)[:, None])
    Q = np.rint(scaled).astype(np.int64)
    assert not exact or np.array_equal(Q.astype(np.float64), scaled), "an entry is rounded by the cut: not a multiple of 2^(e_i - 46)"
    Q0 = Q.copy()
    digs = []
    for _ in range(KMAX):                                                # least significant first, with the carry
        d = ((Q + 128) & 255) - 128
        Q = (Q - d) >> 8
        digs.append(d)
    assert not Q.any(), "more than six planes"
    digs = digs[::-1]
    back = np.zeros_like(Q0)
    for p in range(KMAX):
        back += digs[p] << (8 * (KMAX - 1 - p))
    assert np.array_equal(back, Q0)
    return e, np.stack(digs) if n else np.zeros((KMAX, 0, 0), dtype=np.int64)


def used_planes(M):
    """The 1-based planes of M that hold a non-zero digit."""
    _, d = planes(M)
    return [p + 1 for p in range(KMAX) if d[p].any()]


def plane_pairs(A, B):
    """Non-empty plane pairs of the product off(A) off(B)^T: (p, q) with a non-zero digit on plane p of A and on plane q of B."""
    return {(p, q) for p in used_planes(A) for q in used_planes(B)}


def _matmul_nt(A, B):
    """A B^T exactly in int64, row by row over the non-zeros of A; a Python-int bound rules the wrap-around out first."""
    n = A.shape[0]
    out = np.zeros((n, B.shape[0]), dtype=np.int64)
    if n == 0:
        return out
    nnz = int(np.count_nonzero(A, axis=1).max(initial=0))
    assert int(np.abs(A).max(initial=0)) * int(np.abs(B).max(initial=0)) * max(nnz, 1) < (1 << 62)
    Bt = np.ascontiguousarray(B.T)
    for i in range(n):
        for l in np.flatnonzero(A[i]):
            out[i] += A[i, l] * Bt[l]
    return out


def _wide_pairs(n):
    """The matched pairs (c, c') of wide rows: indices = 3, 11 mod 16, which no multiple of 128 and none of the shapes' last rows touches."""
    if n < 12:
        return []
    pairs = [(3, 11)]
    if n >= 64:
        t = (n // 2) // 16
        pairs.append((16 * t + 3, 16 * t + 11))
    return pairs


def boundary_pairs(n):
    """(j, k), j < k: the corners, the last real row and column, both sides of every multiple of 128 (the 256 and 384 tile edges)."""
    want = [(0, 1), (0, n - 1), (n - 2, n - 1)] + [(b - 1, b) for b in range(128, n, 128)]
    out = []
    for j, k in want:
        if 0 <= j < k < n and (j, k) not in out:
            out.append((j, k))
    return out


def _set(M, j, k, x):
    M[j, k] = M[k, j] = x


def _build_s1(n, rng):
    S = np.zeros((n, n), dtype=np.int64)
    V = np.zeros((n, n), dtype=np.int64)
    wide = _wide_pairs(n)
    C = sorted(c for p in wide for c in p)
    NC = [i for i in range(n) if i not in C]
    e = {}
    for t, i in enumerate(NC):
        e[i] = 6 + (t // 2) % 3
    if len(NC) % 2 and len(NC) >= 3:
        e[NC[-1]] = e[NC[-2]]
    # S: the entry that fixes e_i, then about 32 entries per row and the boundary pairs, each a multiple of the unit of BOTH its rows
    fixed = [(NC[t], NC[t + 1]) for t in range(0, len(NC) - 1, 2)]
    if len(NC) % 2 and len(NC) >= 3:
        fixed.append((NC[-2], NC[-1]))
    for t, (j, k) in enumerate(fixed):
        _set(S, j, k, (63 << (e[j] - 6)) * (1 if t % 2 else -1))
    K = min(16, len(NC) - 1)
    cand = [(i, int(l)) for i in NC for l in rng.choice(NC, size=K, replace=False)] if len(NC) > 1 else []
    for j, k in cand + [p for p in boundary_pairs(n) if p[0] in e and p[1] in e]:
        if j == k or S[j, k]:
            continue
        hi, lo = max(e[j], e[k]), min(e[j], e[k])
        mmax = 63 >> (hi - lo)
        m = int(rng.integers(1, mmax + 1)) * (1 if rng.integers(2) else -1)
        _set(S, j, k, m << (hi - 6))
    for i in NC:
        S[i, i] = int(rng.integers(8, 17)) << (e[i] - 6)
    for c in C:
        S[c, c] = 1 << 12
    # V: the wide pairs (plane 1 = 100, edge digits below), their patterned entries, a ring of plane-3 digits, patterned boundary pairs
    edge = [d for d in EDGE_DIGITS]
    for w, (c, cp) in enumerate(wide):
        _set(V, c, cp, (100 * 65536 + edge[(2 * w) % 6] * 256 + edge[(2 * w + 1) % 6]) * (1 if w % 2 else -1))
    nz = [d for d in EDGE_DIGITS if d]
    for t in range(len(NC) - 1):
        _set(V, NC[t], NC[t + 1], nz[t % 5])
    big2 = [(-128, 127), (-127, -128), (127, -1), (-128, -127), (127, 127), (-127, 1), (-128, -128), (127, -127)]
    small2 = [(-1, 127), (1, -1), (0, 1), (1, -128), (-1, -127), (0, -128), (1, 127), (-1, 1)]
    for w, c in enumerate(C):
        cols = [NC[(37 * w + 101 * u + 5) % len(NC)] for u in range(6)]
        pats = [big2[(2 * w) % 8], big2[(2 * w + 1) % 8]] + [small2[(4 * w + u) % 8] for u in range(4)]
        for l, (d2, d3) in zip(cols, pats):
            _set(V, c, l, d2 * 256 + d3)
    for t, (j, k) in enumerate(boundary_pairs(n)):
        if j in C or k in C:
            continue
        d2, d3 = big2[t % 8] if t % 3 == 0 else small2[t % 8]
        if np.count_nonzero(np.abs(V[j]) >= 32000) >= 2 or np.count_nonzero(np.abs(V[k]) >= 32000) >= 2:
            d2, d3 = small2[t % 8]
        _set(V, j, k, d2 * 256 + d3)
    for i in NC:
        V[i, i] = int(rng.integers(2048, 4097))
    for c in C:
        V[c, c] = 1 << 26
    return S, V, C


def _build_s2(n, rng):
    S = np.zeros((n, n), dtype=np.int64)
    V = np.zeros((n, n), dtype=np.int64)
    wide = _wide_pairs(n)
    C = sorted(c for p in wide for c in p)
    NC = [i for i in range(n) if i not in C]
    fixed = [(NC[t], NC[t + 1]) for t in range(0, len(NC) - 1, 2)]
    if len(NC) % 2 and len(NC) >= 3:
        fixed.append((NC[-2], NC[-1]))
    for t, (j, k) in enumerate(fixed):                                   # about 2^14.2: e = 14, the unit of plane 2 is 1
        _set(S, j, k, ((66 + t % 16) * 256 + EDGE_DIGITS[t % 6]) * (1 if t % 2 else -1))
    K = min(16, len(NC) - 1)
    cand = [(i, int(l)) for i in NC for l in rng.choice(NC, size=K, replace=False)] if len(NC) > 1 else []
    t = 0
    for j, k in cand + [p for p in boundary_pairs(n) if p[0] not in C and p[1] not in C]:
        if j == k or S[j, k]:
            continue
        if t % 7 == 3:
            x = int(rng.integers(-2, 2)) * 256 + 128                    # = 128 mod 256: digit -128 and a carry into plane 1
        else:
            x = int(rng.integers(-2, 3)) * 256 + EDGE_DIGITS[t % 6]
        t += 1
        _set(S, j, k, x if x else 257)
    for i in NC:
        S[i, i] = int(rng.integers(1024, 2049))
    for c in C:
        S[c, c] = 1 << 16
    for t in range(len(NC) - 1):
        _set(V, NC[t], NC[t + 1], 1 if t % 3 else -1)
    for j, k in boundary_pairs(n):
        if not V[j, k] and j not in C and k not in C:
            _set(V, j, k, -1)
    for w, (c, cp) in enumerate(wide):
        _set(V, c, cp, 3 if w else -2)
        _set(V, c, NC[(53 * w + 7) % len(NC)], 1)
        _set(V, cp, NC[(59 * w + 19) % len(NC)], -1)
    V[np.arange(n), np.arange(n)] = 1
    for c in C:
        V[c, c] = 1 << 18
    return S, V, C


def build_case(n, kind, seed=0):
    """-> dict(n, np, kind, S, V, ahat: float64 images zero-padded to np = pad256(n) the way DeviceShard.set_operands pads; Si, Vi, ai: the
    same values as int64 (n x n, n); wide: the rows of S without an off-diagonal part)."""
    assert kind in ("s1", "s2")
    rng = np.random.default_rng(7919 * n + (1 if kind == "s1" else 2) + 104729 * seed)
    Si, Vi, C = (_build_s1 if kind == "s1" else _build_s2)(n, rng)
    ai = rng.integers(-8, 9, size=n).astype(np.int64)
    assert np.array_equal(Si, Si.T) and np.array_equal(Vi, Vi.T)         # exactly symmetric: the asymmetry term of the bound is 0
    assert np.all(np.diag(Si) > 0) and np.all(np.diag(Vi) > 0)
    np_ = pad256(n)
    out = dict(n=n, np=np_, kind=kind, Si=Si, Vi=Vi, ai=ai, wide=C)
    for name, M in (("S", Si), ("V", Vi)):
        P = np.zeros((np_, np_), dtype=np.float64)
        P[:n, :n] = M
        assert np.array_equal(P[:n, :n].astype(np.int64), M)
        out[name] = P
    a = np.zeros(np_, dtype=np.float64)
    a[:n] = ai
    out["ahat"] = a
    return out


def fold(W):
    """W_jj on the diagonal, 2 W_jk above it, 0 below."""
    return 2 * np.triu(W, 1) + np.diag(np.diag(W))


def check_exact(case):
    """-> dict(X = S V^T, W = S X^T, fold, v = S a_hat, r = S (V (S 1)) as int64 (n), Wu / tmp / vv: the float64 images padded to np, pairs1
    of (S, V), pairs2 of (S, X), total = 1^T |S| |V| |S| 1).  Asserts that every value and every partial sum any evaluation order can form
    is below 2^53 units of its last bit (a factor 4 of room for the digit parts of an entry, as tests/exact_scan.py reasons)."""
    S, V, a, n, np_ = case["Si"], case["Vi"], case["ai"], case["n"], case["np"]
    X = _matmul_nt(S, V)
    W = _matmul_nt(S, X)
    aS, aV = np.abs(S), np.abs(V)
    aX = _matmul_nt(aS, aV)
    aW = _matmul_nt(aS, aX)
    # element-wise terms and products: sums of subsets of |S_il| |V_kl| resp. |S_il| |X_jl| (the unit is 1: all operands are integers)
    assert 4 * int(aX.max(initial=0)) < LIMIT and 4 * int(aW.max(initial=0)) < LIMIT
    assert np.all(np.abs(X) <= aX) and np.all(np.abs(W) <= aW)
    # level combine: sum_t 256^-t L_t with |L_t| <= n_pad 128^2 pairs(t) on levels 2..T <= 4: an integer multiple of the last level's unit
    assert np_ * 128 * 128 * 3 * (1 + 256 + 65536) < LIMIT
    # the folded entries 2 W_jk, the vectors, and m^T S (V (S m)) of ANY m in {-1, 0, 1}^n: all below 1^T |S| |V| |S| 1
    total = sum(int(x) for x in aW.sum(axis=1))
    assert 2 * total < 2 * LIMIT and total < LIMIT
    v = S @ a
    assert int(np.abs(aS @ np.abs(a)).max(initial=0)) < LIMIT
    r = S @ (V @ (S @ np.ones(n, dtype=np.int64)))
    Wf = fold(W)
    out = dict(X=X, W=W, fold=Wf, v=v, r=r, total=total, pairs1=plane_pairs(S, V), pairs2=plane_pairs(S, X))
    for name, M in (("Wu", Wf), ("tmp", X)):
        P = np.zeros((np_, np_), dtype=np.float64)
        P[:n, :n] = M
        assert np.array_equal(P[:n, :n].astype(np.int64), M)
        out[name] = P
    vv = np.zeros(np_, dtype=np.float64)
    vv[:n] = v
    out["vv"] = vv
    return out


def vara_truth(case, rows):
    """m^T S (V (S m)) of the int8 rows (count x n) in int64: exact for every row in {-1, 0, 1}^n (check_exact: total < 2^53)."""
    M = np.asarray(rows, dtype=np.int64)
    S, V = case["Si"], case["Vi"]
    T = M @ S.T
    U = T @ V.T
    R = U @ S.T
    return (M * R).sum(axis=1)


def truth_fraction(case, elements):
    """W[j][k] of the listed elements as a triple sum in Fraction."""
    S, V, n = case["Si"], case["Vi"], case["n"]
    out = []
    for j, k in elements:
        w = Fraction(0)
        for l in np.flatnonzero(S[j]):
            x = sum(Fraction(int(S[k, m])) * int(V[l, m]) for m in np.flatnonzero(S[k]))
            w += Fraction(int(S[j, l])) * x
        out.append(w)
    return out


def level_model(A, B, k, T, drop=None, digits_a=None, e_a=None, digits_b=None):
    """The engine's product off(A) off(B)^T from digit planes under configuration (k, T), in int64 units of 2^(e_i + f_j + 4 - 8 T) per
    element -> (G as float64, exact when the result holds).  drop = (p, q, ti, tj): that 256 x 256 tile pair of that plane pair is left
    out; digits_a / digits_b / e_a replace the planes of A / B, the exponents of A (the mutations of the sensitivity tests)."""
    ea, da = planes(A)
    eb, db = planes(B)
    if digits_a is not None:
        da = digits_a
    if e_a is not None:
        ea = e_a
    if digits_b is not None:
        db = digits_b
    n = A.shape[0]
    acc = np.zeros((n, n), dtype=np.int64)
    for p in range(1, k + 1):
        for q in range(1, k + 1):
            if p + q > T:
                continue
            # digits are below 2^7 in magnitude: sums of n products stay far below 2^53, the float64 product is exact
            part = (da[p - 1].astype(np.float64) @ db[q - 1].T.astype(np.float64)).astype(np.int64)
            if drop is not None and drop[:2] == (p, q):
                ti, tj = drop[2:]
                part[256 * ti:256 * ti + 256, 256 * tj:256 * tj + 256] = 0
            acc += part << (8 * (T - p - q))
    return np.ldexp(acc.astype(np.float64), (ea[:, None] + eb[None, :] + 4 - 8 * T))
