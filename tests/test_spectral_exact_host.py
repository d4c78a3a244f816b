"""What tests/test_gpu_spectral_exact.py calls the truth, pinned without a GPU (tests/exact_spectral.py): the construction is exact (the
bounds hold in Python ints for every case the GPU file uses), the int64 truth is the definition in Fraction, a float64 numpy evaluation in
two summation orders returns exactly the truth's doubles, and the assertions the GPU file uses name the marker when the restatement is
deliberately broken."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import exact_spectral as xs


@functools.lru_cache(maxsize=None)
def _case(n, L):
    return xs.build_case(n, L)


def _ops(case):
    """Every operand set the GPU file runs on this case."""
    ops = [("p=%d" % p, xs.single_op(case, p)) for p in xs.single_ps(case)]
    if (case["n"], case["L"]) in xs.TRAIT_SHAPES:
        for k, (plist, _) in enumerate(xs.TRAIT_LISTS):
            ops += [("list %d trait %d" % (k, t), xs.trait_op(case, t, p)) for t, p in enumerate(plist)]
    return ops


@pytest.mark.parametrize("n,L", xs.SHAPES)
def test_construction_is_exact_and_float64_returns_the_truth_in_two_orders(n, L):
    case = _case(n, L)
    U16 = case["U16"]
    Uf = U16.astype(np.float64)                                                     # integers below 2^16: the fp64 product is exact
    np.testing.assert_array_equal(Uf.T @ Uf, 256.0 * np.eye(n))                    # U^T U = I (in Fraction below, small n)
    assert set(np.unique(np.abs(U16))) <= {0, 1, 2, 4, 8, 16} and np.array_equal(case["U"] * 16.0, U16)
    assert sorted(xs.block_sizes(n), reverse=True)[0] == max(b for b in xs.BLOCKS if b <= n)
    if n >= 255:
        assert case["Xp"].shape[1] == 31 and len(set(case["c"])) == 4               # p = 31 fits, all four d values in use
    ops = _ops(case)
    assert ops
    for name, op in ops:
        xs.check_exact(case, op)
        tr = xs.truth(case, op)
        for order in (0, 1):
            Z, a, vara = xs.restate(case, op, order=order)
            what = "n=%d L=%d %s order %d" % (n, L, name, order)
            xs.assert_z(Z, case, what)
            xs.assert_scan(a, vara, tr, what)
            xs.assert_planted(a, vara, case, op, tr, what)
            xs.assert_argmax(*xs.host_argmax(a, vara), tr, what)
        if case["inmodel"] is not None:                                             # r = 0 exactly, and its neighbour r > 0
            assert tr["in_model"][case["inmodel"]] and not tr["in_model"][case["neighbour"]] and tr["r_int"][case["neighbour"]] > 0
        if case["dup"] is not None and n >= 255 and op["y"] is case["y0"]:
            assert tr["argmax"][0] == 1, "construction: the duplicated pair holds the maximum and its first index wins"
            assert tr["a"][0] == tr["a"][L - 1] and tr["vara"][0] == tr["vara"][L - 1]
    if L >= xs.SPECIAL + 8 and n > 2 and n != 256:
        assert case["inmodel"] == L - 3 and case["neighbour"] == L - 2 and case["dup"] == (0, L - 1)


@pytest.mark.parametrize("n,L,p,g", [(43, 30, 9, 0), (43, 30, 1, 1), (23, 20, 5, -1), (2, 20, 1, 2), (1, 3, 1, 0)])
def test_int64_truth_is_the_definition_in_fraction(n, L, p, g):
    case = xs.build_case(n, L)
    p = min(p, case["Xp"].shape[1])
    op = xs.make_op(case, list(range(1, p)) + [0], case["y0"], g)
    xs.check_exact(case, op)
    U = [[Fraction(int(v), 16) for v in row] for row in case["U16"]]
    for j in range(n):
        for k in range(n):
            assert sum(U[i][j] * U[i][k] for i in range(n)) == int(j == k)
    # C and c1 of the library's host operands, restated in Fraction, are the planned dyadic values
    d, Cm, c1 = xs.fraction_operands(case, op)
    assert [Fraction(float(x)) for x in op["d"]] == d and set(d) <= {Fraction(1, 2 ** i) / 4 ** g for i in range(4)}
    for j in range(p):
        assert [Fraction(float(x)) for x in op["C"][j]] == Cm[j] and Fraction(float(op["c1"][j])) == c1[j]
        assert Cm[j][j] == Fraction(2) ** int(op["cexp"][j]) and all(Cm[j][l] == 0 for l in range(p) if l != j)
    tr = xs.truth(case, op)
    for i, (z, fa, fv) in enumerate(xs.truth_fraction(case, op, range(L))):
        assert [Fraction(float(x)) for x in case["Z"][i]] == z, i
        assert Fraction(float(tr["a"][i])) == fa and Fraction(float(tr["vara"][i])) == fv, i
        assert fa == Fraction(op["varG"]) * int(tr["a_int"][i]) * Fraction(2) ** tr["Ea"], i
        assert fv == Fraction(op["varG"]) ** 2 * int(tr["r_int"][i]) * Fraction(2) ** tr["Er"], i
        assert (fa == 0 and fv == 0) == bool(tr["in_model"][i]), i
    if case["inmodel"] is not None:
        assert tr["in_model"][case["inmodel"]] and tr["vara"][case["neighbour"]] == op["varG"] ** 2 * op["d"][case["spare_k"]]
    # masking: exactly those rows become 0 / 0 and leave the arg-max
    trm = xs.truth(case, op, sel=(0, L - 1))
    assert trm["vara"][0] == 0.0 and trm["a"][L - 1] == 0.0 and trm["argmax"][0] not in (1, L)
    np.testing.assert_array_equal(trm["vara"][1:L - 1], tr["vara"][1:L - 1])


def test_trait_lists_produce_every_group_width():
    """spectral_trait_groups restated: the lists of the batched GPU test run k_spectral_scan_traits<NT> for every NT = 2..8, one group with two
    quad tiles (more than 16 traits)."""
    seen = set()
    for plist, widths in xs.TRAIT_LISTS:
        groups = xs.trait_groups(plist)
        assert [g[3] for g in groups] == widths, (plist, groups)
        assert all(1 <= g[2] < g[3] <= 8 for g in groups) and [g[0] for g in groups[1:]] == [g[1] for g in groups[:-1]]
        seen.update(g[3] for g in groups)
    assert seen == {2, 3, 4, 5, 6, 7, 8}
    g0 = xs.trait_groups(xs.TRAIT_LISTS[0][0])[0]
    assert g0[1] - g0[0] > 16 and g0[3] - g0[2] == 2
    assert xs.trait_groups([31]) == [(0, 1, 2, 3)] and xs.trait_groups([1] * 3) == [(0, 3, 1, 2)]
    # traits of one list differ in d: a quad column taken from the neighbouring trait cannot match
    case = _case(257, 257)
    ops = [xs.trait_op(case, t, p) for t, p in enumerate(xs.TRAIT_LISTS[0][0])]
    assert all(not np.array_equal(ops[t]["d"], ops[t + 1]["d"]) for t in range(len(ops) - 1))


@pytest.mark.parametrize("mutate", ["drop_k256", "shift_d", "swap_quad"])
def test_a_broken_restatement_is_named_by_marker(mutate):
    """Self-check of the assertions, on the CPU: one line of the numpy restatement broken (k = 256 dropped at the chunk edge, d shifted by one
    place, the quad column of the neighbouring trait) fails assert_scan with the first wrong marker in the message."""
    case = _case(1003, 257)
    op, other = xs.trait_op(case, 0, 16), xs.trait_op(case, 1, 16)
    tr = xs.truth(case, op)
    Z, a, vara = xs.restate(case, op)
    xs.assert_scan(a, vara, tr, "intact")
    Z, a, vara = xs.restate(case, op, mutate=mutate, quad_d=other["d"])
    bad = np.flatnonzero(~((a == tr["a"]) & (vara == tr["vara"])))
    assert bad.size > 0
    with pytest.raises(AssertionError, match=r"first marker %d:" % bad[0]):
        xs.assert_scan(a, vara, tr, mutate)
    if mutate == "drop_k256":                                                       # only the markers with z_256 != 0 can notice
        assert set(bad.tolist()) <= set(np.flatnonzero(case["Z16"][:, 256]).tolist())
    # a wrong element of Z is named by marker and k
    Zb = case["Z"].copy()
    Zb[129, 256] += 1.0 / 16
    with pytest.raises(AssertionError, match="first marker 129 k 256"):
        xs.assert_z(Zb, case, "Z")
