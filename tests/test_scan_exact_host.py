"""What tests/test_gpu_scan_exact.py calls the truth, pinned without a GPU (tests/exact_scan.py): on operands whose products are exact
the int64 restatement of a_i = sum_j m_ij v_j and vara_i = sum_j W_jj m_ij^2 + 2 sum_{j<k} W_jk m_ij m_ik equals a triple loop in
Fraction, and the fp64 oracle -- a different summation order -- returns exactly the same doubles."""
from fractions import Fraction

import numpy as np
import pytest

import exact_scan as ex


@pytest.mark.parametrize("log2u,s", [(0, 1), (-8, 1), (-16, 1), (-24, 1), (-8, 2)])
def test_int64_truth_is_the_rational_sum_and_the_oracle_is_exact_on_it(log2u, s, oracle):
    n, L = 37, 60
    case = ex.build_case(n, L, log2u=log2u, s=s)
    ex.check_exact(case)
    assert case["probes"] and case["dup"] == (0, L - 1) and case["max_pair"] is not None
    a, vara, units = ex.scan_truth(case)
    frac = ex.scan_truth_fraction(case, range(L))
    for i, (fa, fv) in enumerate(frac):
        assert Fraction(a[i]) == fa and Fraction(vara[i]) == fv, i
        assert Fraction(int(units[i])) * Fraction(2) ** log2u * s * s == fv, i
    # the probe identities: vara(e_j + e_k) - vara(e_j - e_k) = 4 W_jk and vara(e_j) = W_jj
    u = Fraction(2) ** log2u * s * s
    for (j, k), (rp, rm, r1) in case["probes"].items():
        assert frac[rp][1] - frac[rm][1] == 4 * int(case["X"][j, k]) * u, (j, k)
        assert frac[r1][1] == int(case["X"][j, j]) * u, (j, k)
    assert vara[case["zero"]] == 0.0 and a[case["zero"]] == 0.0 and np.all(np.delete(vara, case["zero"]) > 0.0)
    a_o, v_o = oracle.scan_from_i8(case["Mt8"], case["S"], case["V"], case["ahat"])
    np.testing.assert_array_equal(a_o, a)
    np.testing.assert_array_equal(v_o, vara)
    # the arg-max in rationals: first index of the duplicated pair, the oracle's pick, its maximum within one rounding of the division
    idx, best = ex.argmax_truth(a, units, case)
    _, idx_o, mx_o = oracle.tsq_argmax(a_o, v_o)
    assert idx == idx_o == 1 and frac[0] == frac[L - 1]
    assert ex.ulp_distance(mx_o, float(best)) <= 1


def test_edge_values_and_digit_residual():
    ev = ex.edge_values()
    assert len(ev) == len(set(ev)) and all(abs(x) <= ex.MAXOFF and x != 0 for x in ev) and set(ev) == {-x for x in ev}
    for x in (127 * 256 - 128, -128 * 256 + 127, 65536 - 128 * 256 - 128, 127, -128, 65536 + 127 * 256 + 127):
        assert x in ev, x
    # three digits cut from operands that need four: the residual is the balanced low digit of the folded entry (ties to even)
    case = ex.build_case(37, 60, log2u=-8)
    r = ex.digit_residual_units(case, 3, 23)                             # unit 2 = 2^9 u: the folded entries 2 x, in units of u, leave their balanced residue mod 512
    Xf = np.triu(ex.fold_units(case), 1)
    assert np.all(np.abs(r) <= 256) and np.all((Xf - r) % 512 == 0) and np.count_nonzero(r) > 0.9 * 37 * 36 / 2
    assert not ex.digit_residual_units(case, 4, 23).any()
    assert (ex.planted_pairs(1003)[:7] == [(0, 1), (0, 1002), (1001, 1002), (255, 256), (383, 384), (511, 512), (767, 768)])
