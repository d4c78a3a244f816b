"""Operands of the eigenbasis scan (include/eagle_hip.h section 1d) whose Z, lin, quad, a and vara are dyadic rationals that fp64 holds, and
that truth restated without the library (not a conftest; shared by tests/test_spectral_exact_host.py, which pins it on the CPU, and
tests/test_gpu_spectral_exact.py).

    U = P_r blockdiag(H_b / sqrt(b)) P_c, random column signs, b in {256, 64, 16, 4, 1} (Sylvester Hadamard): orthogonal, every entry one bit
                                  ->  Z = Mt U in units of 1/16, |z| <= 16; six int8 digit slices hold U exactly
    h_k = varE + varG lambda_k = 4^g 2^c_k, c_k in 0..3  ->  d_k = 4^-g {1, 1/2, 1/4, 1/8}, varying along k (g = 0 in the single scan)
    Uty integer, |.| <= 8;  UtX in {0, +-1}, supports pairwise disjoint, each inside one d class, s d = 4^m
                                  ->  X^T D X = diag(4^m): the long double Cholesky of the library is exact, C = diag(4^-m), c1 dyadic

    quad_i = sum_k z_ik^2 d_k,  lin_i = z_i^T [d o Uty | d o UtX],  q_i = lin_i[1..p]
    r_i = quad_i - q_i^T C q_i,  vara_i = varG^2 r_i,  a_i = varG (lin_i0 - q_i . c1),  both 0 unless r_i > 1e-12 quad_i          (truth)

truth() evaluates this in int64 on Z16 = 16 Z and D8 = 8 4^g d in one common unit per result; check_exact() bounds, in Python ints, the sum
of the absolute values of the terms of quad, of every lin column, of q^T C q with quad and of q . c1 with lin_0 by 2^53 of that unit (and so
int64 cannot overflow either): every partial sum of every evaluation order, fused or not, is then a double, and every kernel must return the
same bits.  truth_fraction() is the same definition as plain loops in Fraction, with C from a Fraction inverse; the host test holds the int64
form to it.  The limit of the construction: U is block-Hadamard, not a generic eigenbasis, and C is diagonal -- rounding behaviour on generic
operands stays with the tolerance tests."""
from fractions import Fraction

import numpy as np

import exact_scan as ex

BLOCKS = (256, 64, 16, 4, 1)
POOL = 31                                                                # columns of U^T X a case offers (the library's limit on p)
VARE, VARG = 1.0, 2.0                                                    # of g = 0: h_k = 1 + 2 lambda_k = 2^c_k for lambda_k = (2^c_k - 1) / 2
SPECIAL = 6                                                              # planted rows at the end of the panel


def hadamard(b):
    H = np.ones((1, 1), dtype=np.int64)
    while H.shape[0] < b:
        H = np.block([[H, H], [H, -H]])
    return H


def block_sizes(n):
    """n greedily in 256, 64, 16, 4, 1; a 4 is cut into 1 x 1 blocks when fewer than two would be left (the in-model marker and its neighbour
    live on 1 x 1 blocks).  n = 256, 257, 385 keep their 256 block and have 0, 1, 1 of them."""
    out, r = [], n
    for b in BLOCKS:
        while r >= b:
            out.append(b)
            r -= b
    if out.count(1) < 2 and 4 in out:
        out.remove(4)
        out += [1] * 4
    return out


def build_case(n, L, seed=0):
    """-> dict(Mt8 L x n int8, U n x n float64, U16 = 16 U int64, Z16 = 16 Mt U int64, Z, c (d class per k), lam, Xp n x P int64 (the pool of
    U^T X columns, column 0 the in-model one), y0 (Uty of the single scan), zero, plus, minus, inmodel, neighbour, spare_k, dup, n, L)."""
    rng = np.random.default_rng(1000003 * n + 1009 * L + 7919 * seed + 5)
    rowp, colp = rng.permutation(n), rng.permutation(n)
    U16 = np.zeros((n, n), dtype=np.int64)
    ones, o = [], 0                                                      # (individual, k) of the 1 x 1 blocks
    for b in block_sizes(n):
        sg = rng.choice(np.array([-1, 1]), size=b)
        U16[np.ix_(rowp[o:o + b], colp[o:o + b])] = hadamard(b) * sg[None, :] * (16 >> (b.bit_length() - 1) // 2)
        if b == 1:
            ones.append((int(rowp[o]), int(colp[o])))
        o += b
    c = rng.integers(0, 4, size=n)
    k0 = ones[0][1] if ones else None
    k1 = ones[1][1] if len(ones) > 1 else None
    if k0 is not None:
        c[k0] &= 2                                                       # s = 1 needs d = 1 or 1/4
    # the pool of U^T X columns: disjoint supports, each inside one d class, s d = 4^m, at most two thirds of the k in use
    Xp = np.zeros((n, POOL), dtype=np.int64)
    avail = [[int(k) for k in rng.permutation(np.flatnonzero(c == cl)) if k not in (k0, k1)] for cl in range(4)]
    used, P = 0, 0
    if k0 is not None:
        Xp[k0, 0] = rng.choice([-1, 1])
        used, P = 1, 1
    budget = max(1, 2 * n // 3)
    while P < POOL:
        cl = P % 4
        s = (4, 1, 16, 1)[(P // 4) % 4] if cl % 2 == 0 else (2, 8, 2)[(P // 4) % 3]
        if len(avail[cl]) < s or used + s > budget:
            fit = [(1 if q % 2 == 0 else 2, q) for q in range(4) if len(avail[q]) >= (1 if q % 2 == 0 else 2)]
            fit = [(sz, q) for sz, q in fit if used + sz <= budget]
            if not fit:
                break
            s, cl = fit[P % len(fit)]
        ks = [avail[cl].pop() for _ in range(s)]
        Xp[ks, P] = rng.choice(np.array([-1, 1]), size=s)
        used += s
        P += 1
    Xp = Xp[:, :P]
    # markers: random genotypes, then the planted rows at the end of the panel
    Mt8 = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(L, n), p=[0.2, 0.55, 0.25])
    if not Mt8[0].any():
        Mt8[0, 0] = 1
    out = dict(zero=None, plus=None, minus=None, inmodel=None, neighbour=None, dup=None, spare_k=None)
    if L >= SPECIAL + 8:
        r = L - SPECIAL
        Mt8[r] = 0
        Mt8[r + 1] = 1
        Mt8[r + 2] = -1
        out.update(zero=r, plus=r + 1, minus=r + 2, dup=(0, L - 1))
        Mt8[L - 1] = Mt8[0]                                              # the duplicate of marker 0, which Uty makes the largest tsq
        if P and k0 is not None and n > 1:
            i0 = ones[0][0]
            Mt8[r + 3] = 0
            Mt8[r + 3, i0] = Xp[k0, 0] * np.sign(U16[i0, k0])            # z = column 0 of the pool exactly
            Mt8[r + 4] = Mt8[r + 3]
            if k1 is not None:
                Mt8[r + 4, ones[1][0]] = 1                               # one more individual on a 1 x 1 block outside every support: r = d_k1
                out["spare_k"] = k1
            else:
                Mt8[r + 4, int(np.flatnonzero(np.arange(n) != i0)[0])] = 1   # on a larger block: r > 0, whatever the truth says it is
            out.update(inmodel=r + 3, neighbour=r + 4)
    Z16 = (Mt8.astype(np.float64) @ U16.astype(np.float64)).astype(np.int64)   # integers below 2^13: the fp64 product is exact
    y0 = uty_for(Z16[0], rng)
    lam = (np.ldexp(1.0, c) - 1.0) / 2.0
    out.update(Mt8=np.ascontiguousarray(Mt8), U=U16 / 16.0, U16=U16, Z16=Z16, Z=Z16 / 16.0, c=c, lam=lam, Xp=Xp, y0=y0, n=n, L=L, ones=ones)
    return out


def uty_for(z16row, rng):
    """Integer U^T y, |.| <= 8, aligned with one marker's z so that this marker (and its duplicate) hold the largest tsq."""
    return 6 * np.sign(z16row).astype(np.int64) + rng.integers(-2, 3, size=z16row.size)


def single_op(case, p):
    """The single scan's operands with p columns: p - 1 pool columns, then the in-model column LAST (lin column p: the second MFMA tile at
    p >= 16)."""
    P = case["Xp"].shape[1]
    assert 1 <= p <= P
    return make_op(case, list(range(1, p)) + [0], case["y0"], 0)


def trait_op(case, t, p):
    """Trait t of a batched scan: p - 1 pool columns rotated by t and the in-model column, its own Uty (aligned with marker 0 for even t,
    with another marker for odd t) and its own scale of d: 4^-g, g = 0, 1, -1, 2."""
    P = case["Xp"].shape[1]
    assert 1 <= p <= P
    rng = np.random.default_rng(31 * t + p + 977 * case["n"])
    cols = [1 + (5 * t + i) % (P - 1) for i in range(p - 1)] + [0]
    tgt = 0 if t % 2 == 0 else (7 * t) % case["L"]
    return make_op(case, cols, uty_for(case["Z16"][tgt], rng), (0, 1, -1, 2)[t % 4])


def make_op(case, cols, y, g):
    """-> dict(X n x p int64, y int64, g, varE, varG, d, C, c1 (the planned dyadic values), cexp, b)."""
    e = 2 * g
    X = case["Xp"][:, cols]
    D8 = 8 >> case["c"]                                                  # d = D8 2^-(3 + e)
    sd8 = (np.abs(X) * D8[:, None]).sum(axis=0)
    assert np.all(sd8 > 0) and np.all(sd8 & (sd8 - 1) == 0), "s d must be a power of two"
    cexp = (3 + e) - np.array([int(v).bit_length() - 1 for v in sd8])    # C_jj = 2^cexp_j = 1 / (s_j d_j)
    assert np.all(cexp % 2 == 0), "s d = 4^m: the Cholesky's square roots must be exact"
    b = (X * (D8 * y)[:, None]).sum(axis=0)                              # X^T D y in units of 2^-(3 + e)
    d = np.ldexp(D8.astype(np.float64), -(3 + e))
    varE, varG = VARE * 4.0 ** g, VARG * 4.0 ** g
    assert np.array_equal(1.0 / (varE + varG * case["lam"]), d)
    return dict(X=X, y=np.asarray(y, dtype=np.int64), g=g, e=e, varE=varE, varG=varG, d=d, D8=D8, cexp=cexp, b=b,
                C=np.diag(np.ldexp(1.0, cexp)), c1=np.ldexp(b.astype(np.float64), cexp - (3 + e)))


def _ints(case, op):
    Z16, D8, X, y = case["Z16"], op["D8"], op["X"], op["y"]
    quad = (Z16 * Z16) @ D8                                              # units 2^-(11 + e)
    lin0 = Z16 @ (D8 * y)                                                # units 2^-(7 + e)
    q = Z16 @ (D8[:, None] * X)
    return quad, lin0, q


def truth(case, op, sel=()):
    """-> dict(a, vara float64; a_int, r_int int64 with a = varG a_int 2^Ea, vara = varG^2 r_int 2^Er; in_model; argmax = (1-based first index of
    the largest a^2 / vara in rationals, that maximum as a Fraction) or (0, None)).  sel: masked markers (0-based)."""
    e, cexp = op["e"], op["cexp"]
    minc = int(cexp.min())
    sh = 3 + e - minc
    assert sh >= 0
    quad, lin0, q = _ints(case, op)
    w = np.left_shift(1, cexp - minc).astype(np.int64)
    r_int = (quad << sh) - (q * q) @ w                                   # units 2^Er
    a_int = (lin0 << sh) - (q * op["b"]) @ w                             # units 2^Ea
    Er, Ea = -14 - 2 * e + minc, -10 - 2 * e + minc
    # the rule of the finish kernels, r > 1e-12 quad, in Python ints: r_int 2^Er 10^12 > quad_int 2^-(11 + e)
    in_model = ~(r_int.astype(object) * 10 ** 12 > quad.astype(object) * (1 << sh)).astype(bool)
    assert np.all(r_int >= 0)
    off = in_model.copy()
    off[list(sel)] = True
    r_int[off] = 0
    a_int[off] = 0
    lg = int(np.log2(op["varG"]))
    res = dict(a=np.ldexp(a_int.astype(np.float64), Ea + lg), vara=np.ldexp(r_int.astype(np.float64), Er + 2 * lg), a_int=a_int, r_int=r_int,
               in_model=in_model, Ea=Ea, Er=Er, quad=quad, sh=sh)
    res["argmax"] = ex.argmax_truth(a_int, r_int, {"log2u": Er - 2 * Ea, "s": 1})   # (varG a)^2 / (varG^2 r): varG cancels
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def check_exact(case, op):
    """The bounds of the module docstring in Python ints.  Returns the largest of them (in units of the result it belongs to)."""
    Z16, D8, X, y, e, cexp = case["Z16"], op["D8"], op["X"], op["y"], op["e"], op["cexp"]
    assert np.abs(case["U16"]).max() <= 16 and np.abs(Z16).max(initial=0) <= 256 and np.abs(y).max() <= 8 and np.abs(X).max() <= 1
    assert (np.abs(X).sum(axis=1) <= 1).all(), "supports are disjoint"
    for j in range(X.shape[1]):
        assert len(set(case["c"][np.flatnonzero(X[:, j])])) == 1, "a support inside one d class"
    minc = int(cexp.min())
    sh = 3 + e - minc
    A = np.abs(Z16)
    obj = lambda x: np.asarray(x).astype(object)                         # Python ints from here on
    absquad, abslin0 = obj((Z16 * Z16) @ D8), obj(A @ (D8 * np.abs(y)))
    absq = obj(A @ (D8[:, None] * np.abs(X)))
    w = obj([1 << int(cj - minc) for cj in cexp])
    qcq = (absq * absq * w).sum(axis=1)                                  # bounds every product q_j (C q)_j and their partial sums
    qc1 = (absq * obj(np.abs(op["b"])) * w).sum(axis=1)
    worst = max(int(v) for arr in (absquad, abslin0, absq.max(axis=1), absquad * (1 << sh) + qcq, abslin0 * (1 << sh) + qc1) for v in arr)
    assert worst < (1 << 53), ("not exact in fp64 on these operands", worst.bit_length())
    # the in-model rule is nowhere near its threshold: r = 0, or r > 2e-12 quad (the rounding of 1e-12 quad cannot matter)
    quad, lin0, q = _ints(case, op)
    r_int = obj((quad << sh) - (q * q) @ np.left_shift(1, cexp - minc).astype(np.int64))
    assert np.all((r_int == 0) | (r_int * 10 ** 12 > obj(quad) * (2 << sh)))
    return worst


def fraction_operands(case, op):
    """eagle_spectral_host_operands restated in Fraction: d = 1 / (varE + varG lambda), C = (UtX^T D UtX)^-1 by Gauss-Jordan, c1 = C UtX^T D Uty."""
    n, p = op["X"].shape
    d = [1 / (Fraction(op["varE"]) + Fraction(op["varG"]) * Fraction(float(l))) for l in case["lam"]]
    X = [[int(op["X"][k, j]) for j in range(p)] for k in range(n)]
    A = [[sum(X[k][j] * d[k] * X[k][l] for k in range(n)) for l in range(p)] for j in range(p)]
    bv = [sum(X[k][j] * d[k] * int(op["y"][k]) for k in range(n)) for j in range(p)]
    aug = [A[j] + [Fraction(int(j == l)) for l in range(p)] for j in range(p)]
    for j in range(p):
        piv = next(i for i in range(j, p) if aug[i][j] != 0)
        aug[j], aug[piv] = aug[piv], aug[j]
        aug[j] = [v / aug[j][j] for v in aug[j]]
        for i in range(p):
            if i != j and aug[i][j] != 0:
                aug[i] = [vi - aug[i][j] * vj for vi, vj in zip(aug[i], aug[j])]
    Cm = [row[p:] for row in aug]
    return d, Cm, [sum(Cm[j][l] * bv[l] for l in range(p)) for j in range(p)]


def truth_fraction(case, op, rows):
    """(z, a, vara) of the markers `rows` from the definition, plain loops in Fraction."""
    n, p = op["X"].shape
    d, Cm, c1 = fraction_operands(case, op)
    vG = Fraction(op["varG"])
    res = []
    for i in rows:
        m = [int(x) for x in case["Mt8"][i]]
        z = [sum(Fraction(m[j] * int(case["U16"][j, k]), 16) for j in range(n) if m[j]) for k in range(n)]
        quad = sum(z[k] * z[k] * d[k] for k in range(n))
        lin0 = sum(z[k] * d[k] * int(op["y"][k]) for k in range(n))
        q = [sum(z[k] * d[k] * int(op["X"][k, j]) for k in range(n)) for j in range(p)]
        r = quad - sum(q[j] * Cm[j][l] * q[l] for j in range(p) for l in range(p))
        keep = r > Fraction(1, 10 ** 12) * quad
        res.append((z, vG * (lin0 - sum(q[j] * c1[j] for j in range(p))) if keep else Fraction(0), vG * vG * r if keep else Fraction(0)))
    return res


def restate(case, op, order=0, mutate=None, quad_d=None):
    """The definition in float64 numpy, as the kernels evaluate it (Z, the one pass, the finish step), in summation order 0 (the BLAS's) or 1
    (k in chunks of 37, last chunk first).  mutate: None, "drop_k256" (the pass forgets k = 256), "shift_d" (d one place along), "swap_quad"
    (quad from quad_d, another trait's d).  -> (Z, a, vara)."""
    n = case["n"]
    Mt, U = case["Mt8"].astype(np.float64), case["U"]
    d = op["d"].copy()
    if mutate == "shift_d":
        d = np.roll(d, 1)
    G = np.column_stack([d * op["y"], d[:, None] * op["X"]])
    dq = quad_d.copy() if mutate == "swap_quad" else d.copy()
    if mutate == "drop_k256":
        G[256] = 0.0
        dq[256] = 0.0
    edges = list(range(0, n, 37))[::-1]
    if ("Zf", order) not in case:                                        # Z does not depend on the operands: once per case and order
        if order == 0:
            Z = Mt @ U
        else:
            Z = np.zeros((case["L"], n))
            for j0 in edges:
                Z += Mt[:, j0:j0 + 37] @ U[j0:j0 + 37]
        case[("Zf", order)] = Z
    Z = case[("Zf", order)]
    if order == 0:
        lin, quad = Z @ G, (Z * Z) @ dq
    else:
        lin, quad = np.zeros((case["L"], G.shape[1])), np.zeros(case["L"])
        for k0 in edges:
            lin += Z[:, k0:k0 + 37] @ G[k0:k0 + 37]
            quad += (Z[:, k0:k0 + 37] ** 2) @ dq[k0:k0 + 37]
    q = lin[:, 1:]
    r = quad - np.einsum("ij,jl,il->i", q, op["C"], q)
    in_model = ~(r > 1e-12 * quad)
    a = np.where(in_model, 0.0, op["varG"] * (lin[:, 0] - q @ op["c1"]))
    return Z, a, np.where(in_model, 0.0, op["varG"] ** 2 * r)


def assert_z(Zgot, case, what):
    """Zgot L x n against the truth, every element; the first wrong one named by marker and k."""
    bad = np.argwhere(Zgot != case["Z"])
    assert bad.size == 0, "%s: Z of %d elements, first marker %d k %d: %r, truth %r" % (
        what, bad.shape[0], bad[0, 0], bad[0, 1], Zgot[bad[0, 0], bad[0, 1]], case["Z"][bad[0, 0], bad[0, 1]])


def assert_scan(a_got, v_got, tr, what):
    """a and vara bit for bit; the first wrong marker named."""
    a_got, v_got = np.ravel(a_got), np.ravel(v_got)
    assert a_got.shape == tr["a"].shape and v_got.shape == tr["vara"].shape, what
    bad = np.flatnonzero(~((v_got == tr["vara"]) & (a_got == tr["a"])))
    assert bad.size == 0, "%s: %d markers wrong, first marker %d: a %r vara %r, truth %r %r" % (
        what, bad.size, bad[0], a_got[bad[0]], v_got[bad[0]], tr["a"][bad[0]], tr["vara"][bad[0]])


def assert_planted(a_got, v_got, case, op, tr, what, sel=()):
    """The planted rows by name: zero and in-model markers exactly 0 / 0, the neighbour kept with its exact r (one d_k where a spare 1 x 1
    block exists), the masked rows exactly 0 / 0 and no other row 0 / 0 that the truth does not name."""
    a_got, v_got = np.ravel(a_got), np.ravel(v_got)
    for i in sel:
        assert a_got[i] == 0.0 and v_got[i] == 0.0, "%s: masked marker %d" % (what, i)
    zeros = set(np.flatnonzero((a_got == 0.0) & (v_got == 0.0)).tolist())
    named = set(np.flatnonzero(tr["in_model"]).tolist()) | set(sel)
    assert zeros == named, "%s: 0 / 0 at markers %r, truth %r" % (what, sorted(zeros ^ named)[:5], sorted(named)[:5])
    if case["zero"] is not None:
        assert case["zero"] in named
    if case["inmodel"] is not None:                                      # every op holds pool column 0, the in-model one
        i, nb = case["inmodel"], case["neighbour"]
        assert a_got[i] == 0.0 and v_got[i] == 0.0, "%s: in-model marker %d: %r %r" % (what, i, a_got[i], v_got[i])
        if nb not in sel:
            assert v_got[nb] > 0.0 and v_got[nb] == tr["vara"][nb], "%s: neighbour marker %d: %r, truth %r" % (what, nb, v_got[nb], tr["vara"][nb])
            if case["spare_k"] is not None:
                assert v_got[nb] == op["varG"] ** 2 * op["d"][case["spare_k"]], "%s: neighbour marker %d is not varG^2 d_k" % (what, nb)


def assert_argmax(idx1, tsqmax, tr, what):
    """First index of the exact rational maximum; the value within 2 ulp (one rounding is in the division, and include/eagle_hip.h fixes
    no more than that: the margin tests/test_gpu_scan_exact.py uses)."""
    idx, mx = tr["argmax"]
    assert int(idx1) == idx, "%s: arg-max marker %d, truth %d" % (what, idx1, idx)
    if idx == 0:
        assert np.isnan(tsqmax), what
    else:
        assert ex.ulp_distance(tsqmax, float(mx)) <= 2, (what, tsqmax, float(mx))


def host_argmax(a, vara):
    """find_qtl.R:71-83 as am.SpectralBackend.find_qtl evaluates it on the returned arrays: (1-based first index, maximum) or (0, NaN)."""
    a, vara = np.ravel(a), np.ravel(vara)
    with np.errstate(all="ignore"):
        tsq = a * a / vara
    if np.all(np.isnan(tsq)):
        return 0, np.nan
    mx = np.nanmax(tsq)
    return int(np.flatnonzero(tsq == mx)[0]) + 1, float(mx)


def trait_groups(p, max_tiles=8):
    """spectral_trait_groups (csrc/eagle_host.h) restated: whole traits in order, as many as fit max_tiles MFMA tiles of 16 columns;
    -> [(t0, t1, ntl, nt)]."""
    out, t0, lin = [], 0, 0
    tiles = lambda x: (x + 15) // 16
    for t in range(len(p)):
        lin2 = lin + p[t] + 1
        if t > t0 and tiles(lin2) + tiles(t - t0 + 1) > max_tiles:
            out.append((t0, t, tiles(lin), tiles(lin) + tiles(t - t0)))
            t0, lin = t, p[t] + 1
        else:
            lin = lin2
    if p:
        out.append((t0, len(p), tiles(lin), tiles(lin) + tiles(len(p) - t0)))
    return out


# The shapes of tests/test_gpu_spectral_exact.py.  n: 1, 2, one chunk of 256 less one / exactly / plus one, the digit-slice build's 384 tile plus
# one, four chunks with a ragged last one; L: one marker, the 128 tile of k_zbuild plus one, the 256-marker workgroup plus one, 1,000.
SHAPES = [(1, 1), (1, 129), (2, 129), (2, 1000), (255, 257), (256, 129), (256, 1000), (257, 1), (257, 257), (257, 1000), (385, 129), (385, 1000),
          (1003, 1), (1003, 257), (1003, 1000)]
P_SINGLE = (1, 15, 16, 31)
# p of the traits of each batched call and the group widths nt it must produce: every k_spectral_scan_traits<NT>, NT = 2..8; the first list has
# 19 traits in one group (two quad tiles)
TRAIT_LISTS = [([4] * 20, [8, 2]), ([31, 31, 31, 31, 20], [7, 5]), ([31, 31, 31, 31, 31, 14], [7, 6]), ([31, 31, 31, 31, 5], [7, 4]),
               ([31, 31, 31, 20], [7, 3])]
TRAIT_SHAPES = [(257, 257), (1003, 1000)]


def single_ps(case):
    return [p for p in P_SINGLE if p <= case["Xp"].shape[1]]
