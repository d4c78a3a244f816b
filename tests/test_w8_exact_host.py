"""The exact-integer truth of W = S (V S) with a non-diagonal S (tests/exact_w8.py) pinned on the CPU, before tests/test_gpu_w8_exact.py
asks the device: the constructions hit the plane, carry, exponent and tile edges they claim, their non-empty plane pairs lie inside (3, 4)
-- the cheapest configuration, a subset of all others -- the truth agrees with two independent routes (float64 multi_dot where every sum is
exact, Fraction), the numpy restatement of the digit planes reproduces it through the level sums, single-digit and single-tile mutations of
that model change the folded image -- and, on operands with all six planes in use, stay under a tenth of the library's own bound --
and the work lists of (3, 4) name every upper tile pair of every level group once at the new sizes."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_w8 as ex
from eagleeverything_amd import _lib
from test_gpu_w8_exact import CASES
from test_w8_host import _stats, _work_list


@functools.lru_cache(maxsize=None)
def _case(n, kind):
    case = ex.build_case(n, kind)
    truth = ex.check_exact(case)                                         # the 2^53 bounds, in integers
    return case, truth


def _off(M):
    return M - np.diag(np.diag(M))


@pytest.mark.parametrize("n,kind", CASES)
def test_constructions_are_exact_covered_and_hit_their_edges(n, kind):
    case, truth = _case(n, kind)
    S, V, X, np_ = case["Si"], case["Vi"], truth["X"], case["np"]
    assert ex.covered(truth["pairs1"], 3, 4) and ex.covered(truth["pairs2"], 3, 4)
    assert all(ex.covered(truth["pairs1"] | truth["pairs2"], k, T) for k, T in ex.W8_CONFIGS)
    # padding as DeviceShard.set_operands pads; exactly symmetric
    for M, Mi in ((case["S"], S), (case["V"], V)):
        assert M.shape == (np_, np_) and not M[n:].any() and not M[:, n:].any() and np.array_equal(M[:n, :n], Mi) and np.array_equal(M, M.T)
    assert not truth["Wu"][n:].any() and not truth["Wu"][:, n:].any() and not np.tril(truth["Wu"], -1).any()
    eS, dS = ex.planes(S)
    eV, dV = ex.planes(V)
    eX, dX = ex.planes(X)
    if n == 1:
        assert not truth["pairs1"] and not truth["pairs2"]
        return
    # non-zeros on both sides of every 256 and 384 boundary below n, in the last real row and column
    for M in (S, V):
        for b in range(128, n, 128):
            assert M[b - 1, b] and M[b, b - 1]
        assert _off(M)[n - 1].any() and _off(M)[:, n - 1].any()
    if kind == "s1":
        assert ex.used_planes(S) == [1] and int(np.abs(dS[0]).max()) == 63                     # one plane, |m| <= 63, 63 fixes e_i
        live = np.abs(_off(S)).max(axis=1) > 0
        assert np.all(np.abs(dS[0]).max(axis=1)[live] == 63)
        if n >= 12:
            assert len(set(eS[live].tolist())) >= 3 and len(case["wide"]) >= 2 and not live[case["wide"]].any()
        if n >= 64:   # three planes of V; every edge digit on planes 2 and 3 of the rows whose e = 22 makes them the digits of d2, d3
            assert ex.used_planes(V) == [1, 2, 3] and ex.used_planes(X) == [1, 2, 3]
            wide = np.flatnonzero(eV == 22)
            assert sorted(wide.tolist()) == case["wide"]
            for p in (1, 2):
                assert set(ex.EDGE_DIGITS) <= set(np.unique(dV[p][wide]).tolist()), p
    else:
        assert ex.used_planes(S) == [1, 2] and set(ex.used_planes(X)) <= {1, 2} and ex.used_planes(V) == [1]
        live = np.abs(_off(S)).max(axis=1) > 0
        assert set(eS[live].tolist()) == {14}
        assert set(ex.EDGE_DIGITS) <= set(np.unique(dS[1]).tolist())
        carry = (dS[1] == -128) & (_off(S) % 256 == 128)                                       # +128 is cut as -128 and a carry into plane 1
        assert carry.any() and np.all(dS[0][carry] == (_off(S)[carry] >> 8) + 1)
        assert (carry & (_off(S) > 0) & (dS[0] == 2)).any()                                     # 384 = 2 x 256 - 128
    # both products have non-zeros in every pair of 256-row tiles and of 256 x 384 tiles
    F = _off(S)
    G1 = ex._matmul_nt(F, _off(V))
    G2 = ex._matmul_nt(F, _off(X))
    wide = set(case["wide"])
    for G in (G1, G2):
        for i0 in range(0, n, 256):
            rows = [i for i in range(i0, min(n, i0 + 256)) if i not in wide]
            for tj in (256, 384):
                for j0 in range(0, n, tj):
                    assert len(rows) == 0 or G[rows, j0:j0 + tj].any(), (i0, j0, tj)


@pytest.mark.parametrize("n,kind", [c for c in CASES if c[0] <= 385])
def test_truth_against_float64_and_the_level_sums_of_the_plane_model(n, kind):
    case, truth = _case(n, kind)
    S, V = case["S"][:n, :n], case["V"][:n, :n]
    Wf = np.linalg.multi_dot([S, V, S])                                  # every sum below 2^53: exact in any order
    assert np.array_equal(Wf, truth["W"].astype(np.float64))
    assert np.array_equal(S @ V.T, truth["X"].astype(np.float64)) and np.array_equal(S @ case["ahat"][:n], truth["v"].astype(np.float64))
    assert np.array_equal(S @ (V @ (S @ np.ones(n))), truth["r"].astype(np.float64))
    # the engine's algebra on the restated planes: X = D Dv [j = k] + D_j Fv[k][j] + F[j][k] Dv_k + G1, W likewise from X
    Si, Vi, Xi = case["Si"], case["Vi"], truth["X"]
    d, dv, dx = np.diag(Si).astype(np.float64), np.diag(Vi).astype(np.float64), np.diag(Xi).astype(np.float64)
    F, Fv, Fx = (_off(M).astype(np.float64) for M in (Si, Vi, Xi))
    X = np.diag(d * dv) + d[:, None] * Fv.T + F * dv[None, :] + ex.level_model(Si, Vi, 3, 4)
    assert np.array_equal(X, Xi.astype(np.float64))
    W = np.diag(d * dx) + d[:, None] * Fx.T + F * dx[None, :] + ex.level_model(Si, Xi, 3, 4)
    assert np.array_equal(W, truth["W"].astype(np.float64))
    m = np.ones((1, n), dtype=np.int8)
    assert int(ex.vara_truth(case, m)[0]) == int(truth["W"].sum()) <= truth["total"]


def test_truth_against_fractions():
    case, truth = _case(257, "s2")
    n = case["n"]
    els = [(0, 0), (0, 1), (0, n - 1), (n - 1, n - 1), (255, 256), (3, 11), (3, 3), (127, 128), (40, 200)]
    for (j, k), w in zip(els, ex.truth_fraction(case, els)):
        assert w.denominator == 1 and int(w) == int(truth["W"][j, k]), (j, k)
    case, truth = _case(385, "s1")
    els = [(383, 384), (3, 11), (0, 384), (384, 384), (255, 256)]
    for (j, k), w in zip(els, ex.truth_fraction(case, els)):
        assert int(w) == int(truth["W"][j, k]), (j, k)


@pytest.mark.parametrize("kind", ["s1", "s2"])
def test_single_tile_digit_and_exponent_mutations_change_the_folded_image(kind):
    """What the equality on the whole image catches, on the exact operands themselves: one 256 x 256 tile pair of the least significant plane
    pair dropped, one digit -128 read as +127 (a digit of X for "s1", whose S has no -128 on its single plane; of S for "s2"), the exponent
    of the wrong row -- each changes elements of the folded W, and only where it should.  (On THESE operands the library's bound would see
    them too: nothing is dropped, so it sits at its 2^-49 floor, below one unit.  That the bound on operands with all six planes in use does
    not is test_mutations_stay_under_a_tenth_of_the_bound_on_six_plane_operands.)"""
    case, truth = _case(385, kind)
    Si, Xi, n = case["Si"], truth["X"], case["n"]
    d, dx = np.diag(Si).astype(np.float64), np.diag(Xi).astype(np.float64)
    F, Fx = _off(Si).astype(np.float64), _off(Xi).astype(np.float64)
    base = np.diag(d * dx) + d[:, None] * Fx.T + F * dx[None, :]
    want = ex.fold(truth["W"]).astype(np.float64)
    assert np.array_equal(ex.fold(base + ex.level_model(Si, Xi, 3, 4)), want)
    eS, dS = ex.planes(Si)
    eX, dX = ex.planes(Xi)
    p, q = max(truth["pairs2"], key=lambda t: (t[0] + t[1], t[1]))
    # (a) the tile pair (0, 1) of the least significant non-empty plane pair
    Wa = ex.fold(base + ex.level_model(Si, Xi, 3, 4, drop=(p, q, 0, 1)))
    bad = np.argwhere(Wa != want)
    assert 0 < len(bad) and np.all(bad[:, 0] < 256) and np.all(bad[:, 1] >= 256)
    # (b) one digit -128 read as +127: W changes in the row / column of the entry's row, nowhere else
    if kind == "s2":
        pl = 1
        hit = np.argwhere(dS[pl] == -128)
        i, l = (int(x) for x in hit[len(hit) // 2])
        dm = dS.copy()
        dm[pl][i, l] = 127
        Wb = ex.fold(base + ex.level_model(Si, Xi, 3, 4, digits_a=dm))
    else:
        pl = max(p_ for p_ in range(ex.KMAX) if (dX[p_] == -128).any())
        hit = np.argwhere(dX[pl] == -128)
        i, l = (int(x) for x in hit[len(hit) // 2])
        dm = dX.copy()
        dm[pl][i, l] = 127
        Wb = ex.fold(base + ex.level_model(Si, Xi, 3, 4, digits_b=dm))
    bad = np.argwhere(Wb != want)
    assert 0 < len(bad) and np.all((bad[:, 0] == i) | (bad[:, 1] == i))
    # (c) a row of S cut on the exponent of a row whose e differs
    i = next(int(r) for r in range(n) if eS[r] > 0)
    other = next(int(r) for r in range(n) if eS[r] != eS[i])
    em = eS.copy()
    em[i] = eS[other]
    Wc = ex.fold(base + ex.level_model(Si, Xi, 3, 4, e_a=em))
    bad = np.argwhere(Wc != want)
    assert 0 < len(bad) and np.all((bad[:, 0] == i) | (bad[:, 1] == i))


def _six_plane_operand(n, seed, quiet):
    """Diagonal + an off-diagonal part of random 47-bit integers times 2^(e_i - 46): all six planes of every row in use, cut without rounding,
    e_i = i mod 2; `quiet` {row: e}: rows whose off-diagonal part is that much smaller (a nearly unrelated individual)."""
    rng = np.random.default_rng(seed)
    e = np.arange(n) % 2
    for r, x in quiet.items():
        e[r] = x
    Q = rng.integers(-int(1.9 * 2 ** 46), int(1.9 * 2 ** 46) + 1, size=(n, n))
    M = np.ldexp(Q.astype(np.float64), (e - 46)[:, None])
    np.fill_diagonal(M, 8.0 * rng.uniform(0.5, 1.5, n))
    return M, e


def test_mutations_stay_under_a_tenth_of_the_bound_on_six_plane_operands():
    """Why the equalities are needed.  On operands that use all six planes a configuration drops plane pairs, and the bound the library
    accepts a product with -- eagle_w8_host_bound, its own function, at (3, 5); the eta of W is at least sqrt(2) times it -- pays for all of
    them over the whole matrix.  A fault confined to one tile pair, one digit or one quiet row changes elements of the product and stays
    below a tenth of that bound, so tests/test_gpu_w8.py (|| W8 - W64 ||_F <= eta) passes it.  Figures of this test (n = 512, two 256-row
    tiles; bound 0.0997, the model's own error 0.0031, the 30-fold slack tests/test_gpu_w8.py knows of): one tile pair of plane pair (3, 2)
    dropped 0.0011 = 0.011 bound; a -128 of plane 3 read as +127 0.0024 = 0.024 bound; a row whose off-diagonal part is 2^-18 of the others'
    cut on its neighbour's exponent (one apart) about 0.02 bound.  The third does NOT hold for an ordinary row: the wrong exponent rescales a
    whole row of G, 959 = 9,600 bound, and the bound test catches it -- asserted as such."""
    L = _lib.load()
    n, k, T = 512, 3, 5
    A, eA = _six_plane_operand(n, 1, {300: -18, 301: -19})
    B, _ = _six_plane_operand(n, 2, {})
    e, dA = ex.planes(A)                                                 # exact: no rounding in the cut
    assert np.array_equal(e, eA) and ex.used_planes(A) == ex.used_planes(B) == [1, 2, 3, 4, 5, 6]
    sa, Fa, _, _ = _stats(A)
    sb, Fb, _, _ = _stats(B)
    bound = L.eagle_w8_host_bound(C.byref(sa), C.byref(sb), k, T, n)
    G = ex.level_model(A, B, k, T)
    fro = lambda D: float(np.sqrt((D * D).sum()))
    err = fro(G - Fa @ Fb.T)
    assert 0.0 < err <= bound                                            # the bound is real here: pairs are dropped, and it holds
    # (a) the tile pair (0, 1) of a plane pair of the last level computed
    da = fro(ex.level_model(A, B, k, T, drop=(3, 2, 0, 1)) - G)
    assert 0.0 < da < 0.1 * bound, (da, bound)
    # (b) a digit -128 of the last plane in use, in an ordinary row, read as +127
    i, l = next((int(r), int(c)) for r, c in np.argwhere(dA[k - 1] == -128) if r not in (300, 301))
    dm = dA.copy()
    dm[k - 1][i, l] = 127
    db = fro(ex.level_model(A, B, k, T, digits_a=dm) - G)
    assert 0.0 < db < 0.1 * bound, (db, bound)
    # (c) the exponent of the wrong row: under a tenth of the bound for a quiet row, far above the bound for an ordinary one
    em = eA.copy()
    em[300] = eA[301]
    dc = fro(ex.level_model(A, B, k, T, e_a=em) - G)
    assert 0.0 < dc < 0.1 * bound, (dc, bound)
    em = eA.copy()
    em[10] = eA[11]
    dc = fro(ex.level_model(A, B, k, T, e_a=em) - G)
    assert dc > bound, (dc, bound)


@pytest.mark.parametrize("piped", [0, 1])
@pytest.mark.parametrize("nt", sorted({ex.pad256(n) // 256 for n, _ in CASES}))
def test_work_list_of_the_cheapest_configuration_names_every_upper_tile_pair_once(nt, piped):
    tj_rows = 384 if piped else 256
    ntj = (nt * 256 + tj_rows - 1) // tj_rows
    for upper in (0, 1):
        for rt0, rt1 in {(0, nt), (0, (nt + 1) // 2), ((nt + 1) // 2, nt)}:
            if rt0 >= rt1:
                continue
            wl, groups = _work_list(nt, rt0, rt1, upper, piped, 3, 4, 8)
            assert sorted((g.p[i] + 1, g.q[i] + 1) for g in groups for i in range(g.npairs)) == [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (3, 1)]
            assert [g.level for g in groups] == [2, 3, 4]
            items = [(int(x >> 20), int((x >> 8) & 0xFFF), int(x & 0xFF)) for x in wl[wl != 0xFFFFFFFF]]
            need = {(i, j, g) for i in range(rt0, rt1) for j in range(ntj) for g in range(len(groups))
                    if not upper or j * tj_rows + tj_rows - 1 >= i * 256}
            assert len(items) == len(set(items)) and set(items) == need
