"""CPU: the numpy restatement of the epistasis scan (r_api.epistasis_host, include/eagle_hip.h section 1b''''ii) against plain loops and
exact fractions (tests/epistasis_truth.py), r_api.quantise_trait, and the rules of the all-pairs mode.  No device work.

The tolerance of the statistic is derived, not measured: with u = 2^-53, each of the three t53 truncations errs by less than 2u relative,
each of the six fp64 operations by at most u; r2 collects 2 (2u + 2u + u) + u <= 11u (Sxy enters twice), the numerator (n - 4) r2 one more
u, the quotient one more, and 1 - r2 turns r2's relative error into r2 / (1 - r2) times as much plus u: in all below (13 + 12 r2 / (1 - r2))
u <= 32 u / (1 - r2) relative."""
import math
from fractions import Fraction

import numpy as np
import pytest

import epistasis_truth as truth

U = Fraction(1, 2 ** 53)


def panel(n, L, seed, ymax=1000):
    rng = np.random.default_rng(seed)
    G = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(n, L), p=[0.3, 0.4, 0.3])
    y = rng.integers(-ymax, ymax + 1, n).astype(np.int64)
    return G, y


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def check_stat(stat, t):
    F = truth.exact_F(t)
    if F is None:
        assert math.isnan(stat)
    elif F == "inf":
        assert stat == math.inf
    else:
        r2 = truth.exact_r2(t)
        assert math.isfinite(stat)
        assert abs(Fraction(stat) - F) <= 32 * U / (1 - r2) * F, (stat, float(F), float(r2))


@pytest.mark.parametrize("n,L,seed,ymax", [(5, 6, 1, 7), (6, 7, 2, 1000000), (17, 8, 3, 1000), (64, 9, 4, 1000000), (129, 7, 5, 100), (200, 8, 6, 1000000)])
def test_host_integers_equal_loops_and_stat_within_derived_bound(n, L, seed, ymax):
    from eagleeverything_amd import r_api
    G, y = panel(n, L, seed, ymax)
    loci = [0, L - 1, 2, 2]
    r = r_api.epistasis_host(G, y, loci=loci)
    assert r["stat"].shape == (L, 4) and r["mom"].shape == (L, 4, 5) and r["mom"].dtype == np.int64
    allp = r_api.epistasis_host(G, y, min_stat=-math.inf)
    by_pair = {(int(i), int(j)): k for k, (i, j) in enumerate(allp["hit_ij"])}
    ndef = 0
    for i in range(L):
        for k, j in enumerate(loci):
            t = truth.sums(G[:, i], G[:, j], y)
            assert [int(v) for v in r["mom"][i, k]] == [t["d"], t["e"], t["f"], t["h"], t["z"]]
            D, Sxx, Sxy, Syy = truth.S(t)
            si, qi, ui, sj, qj, uj = (np.array([t[key]]) for key in ("si", "qi", "ui", "sj", "qj", "uj"))
            got = r_api._epi_sums(n, t["Y"], t["T"], (si, qi, ui), (sj, qj, uj), r["mom"][i, k][None, :])
            assert [int(g[0]) for g in got] == [D, Sxx, Sxy, Syy]
            check_stat(float(r["stat"][i, k]), t)
        for j in range(i + 1, L):
            t = truth.sums(G[:, i], G[:, j], y)
            if truth.defined(t):
                ndef += 1
                kk = by_pair[(i, j)]
                check_stat(float(allp["hit_stat"][kk]), t)
                assert [int(v) for v in allp["hit_mom"][kk]] == [t["d"], t["e"], t["f"], t["h"], t["z"]]
            else:
                assert (i, j) not in by_pair
    assert allp["ntested"] == ndef == allp["nhits"]
    for k in (2, 3):                                            # a repeated locus repeats its column
        assert same_bits(r["stat"][:, 2], r["stat"][:, k])


def test_t53_truncates_toward_zero():
    from eagleeverything_amd import r_api
    for x in (0, 1, -1, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 54 + 3, 2 ** 110 - 1, -(2 ** 110 - 1), 3 ** 60, -(3 ** 60)):
        v = r_api._epi_t53(x)
        m = abs(x)
        sh = max(0, m.bit_length() - 53)
        assert Fraction(v) == (1 if x >= 0 else -1) * ((m >> sh) << sh)
        assert abs(Fraction(v)) <= m and (m == 0 or abs(Fraction(v)) > m * (1 - 2 * U))


def test_undefined_pairs_are_nan():
    from eagleeverything_amd import r_api
    G, y = panel(40, 6, 7)
    G[:, 1] = 1                                                 # monomorphic
    G[:, 2] = G[:, 0]                                           # a duplicate of marker 0
    G[:, 3] = -G[:, 0]                                          # and its mirror: g_3 in the span of g_0
    G[:, 4] = np.where(G[:, 5] == 1, G[:, 4], 0)                # g_4 != 0 only where g_5 = 1: g_5 g_4 = g_4, Sxx = 0
    G[:4, 4] = [1, -1, 1, -1]
    G[:4, 5] = 1
    st = r_api.epistasis_host(G, y, loci=list(range(6)))["stat"]
    for i in range(6):
        assert math.isnan(st[i, i])                             # i = j
        assert math.isnan(st[i, 1]) and math.isnan(st[1, i])
    for a, b in ((0, 2), (2, 0), (0, 3), (3, 2), (4, 5), (5, 4)):
        assert math.isnan(st[a, b]), (a, b)
        t = truth.sums(G[:, a], G[:, b], y)
        assert not truth.defined(t)
    assert truth.S(truth.sums(G[:, 5], G[:, 4], y))[1] == 0 and truth.S(truth.sums(G[:, 5], G[:, 4], y))[0] > 0
    assert np.isfinite(st[0, 5]) and np.isfinite(st[5, 0])
    G4, y4 = panel(4, 5, 8)                                     # n = 4: no degree of freedom is left
    assert np.isnan(r_api.epistasis_host(G4, y4, loci=[0, 1])["stat"]).all()
    p4 = r_api.epistasis_host(G4, y4, min_stat=-math.inf)
    assert p4["ntested"] == 0 and p4["nhits"] == 0 and p4["max"][:2] == (-1, -1) and math.isnan(p4["max"][2])


def test_exact_product_trait_is_inf():
    from eagleeverything_amd import r_api
    G, _ = panel(60, 5, 9)
    y = G[:, 1].astype(np.int64) * G[:, 3]                      # y = g_i g_j exactly: Sxy = Sxx = Syy, r2 = 1
    r = r_api.epistasis_host(G, y, loci=[3])
    assert r["stat"][1, 0] == math.inf and truth.exact_F(truth.sums(G[:, 1], G[:, 3], y)) == "inf"
    assert np.isfinite(r["stat"][0, 0])
    # a trait in the span of 1, g_i, g_j: Syy = 0, documented as +inf too
    y2 = 5 + 3 * G[:, 1].astype(np.int64) - 2 * G[:, 3]
    assert r_api.epistasis_host(G, y2, loci=[3])["stat"][1, 0] == math.inf
    assert truth.S(truth.sums(G[:, 1], G[:, 3], y2))[3] == 0


def test_quantise_trait():
    from eagleeverything_amd import r_api, rcpp_api
    rng = np.random.default_rng(10)
    for y in (rng.standard_normal(50), 1e9 + 1e3 * rng.standard_normal(50), 1e-9 * rng.standard_normal(7), np.array([0.0, 1.0]),
              np.array([-3.0, 1.0, 2.0]) * 1e6):
        yq, scale = r_api.quantise_trait(y)
        c = y - y.mean()
        mx = np.abs(c).max()
        assert yq.dtype == np.int32 and np.abs(yq).max() <= rcpp_api.EPI_YMAX
        assert math.frexp(scale)[0] == 0.5 and mx * scale <= rcpp_api.EPI_YMAX < mx * scale * 2       # the largest power of two
        assert np.all(np.abs(c - yq / scale) <= 0.5 / scale) and 0.5 / scale <= 1e-6 * mx
    yq, scale = r_api.quantise_trait(np.full(9, 4.25))
    assert not yq.any() and yq.dtype == np.int32 and scale == 1.0
    with pytest.raises(ValueError):
        r_api.quantise_trait([1.0, np.nan])


def test_stat_is_invariant_to_shift_and_scale():
    from eagleeverything_amd import r_api
    G, y = panel(77, 9, 11, 300000)
    a = r_api.epistasis_host(G, y, loci=[0, 4, 8])
    b = r_api.epistasis_host(G, 2 * y + 3, loci=[0, 4, 8])
    assert same_bits(a["stat"], b["stat"]) and np.isfinite(a["stat"]).sum() > 20


def test_planted_interaction_is_the_maximum():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(12)
    n, L, a, b = 300, 200, 37, 161
    G = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(n, L), p=[0.3, 0.4, 0.3])
    y = rng.standard_normal(n)
    y = y + 0.3 * (y.max() - y.min()) * G[:, a] * G[:, b]
    yq, _ = r_api.quantise_trait(y)
    r = r_api.epistasis_host(G, yq, min_stat=30.0)
    assert r["max"][:2] == (a, b) and r["max"][2] > 100.0
    assert [a, b] in r["hit_ij"].tolist() and r["nhits"] < 10 and r["ntested"] == L * (L - 1) // 2


def test_gap_and_chrom_skip_exactly_the_stated_pairs():
    from eagleeverything_amd import r_api
    G, y = panel(30, 14, 13)
    chrom = np.array([1] * 5 + [2] * 4 + [7] * 5)
    for ch, gap in ((None, 0), (None, 3), (chrom, 3), (chrom, 100), (None, 100), (chrom, 1)):
        r = r_api.epistasis_host(G, y, chrom=ch, gap=gap, min_stat=-math.inf)
        want = [[i, j] for i in range(14) for j in range(i + 1, 14)
                if truth.pair_tested(i, j, None if ch is None else list(ch), gap) and truth.defined(truth.sums(G[:, i], G[:, j], y))]
        assert r["hit_ij"].tolist() == want and r["ntested"] == len(want)
    assert r_api.epistasis_host(G, y, gap=100)["ntested"] == 0
    assert r_api.epistasis_host(G, y, chrom=chrom, gap=100)["ntested"] == 91 - 10 - 6 - 10


def test_hit_cap_semantics_and_maximum_ties():
    from eagleeverything_amd import r_api
    G, y = panel(50, 10, 14)
    G[:, 7] = G[:, 2]                                           # (0, 2) and (0, 7) tie, like every (k, 2) and (k, 7)
    full = r_api.epistasis_host(G, y, min_stat=1.0)
    assert 0 < full["nhits"] < full["ntested"] and np.all(full["hit_stat"] >= 1.0)
    ij = full["hit_ij"].tolist()
    assert ij == sorted(ij)
    at = r_api.epistasis_host(G, y, min_stat=1.0, hit_cap=full["nhits"])
    assert np.array_equal(at["hit_ij"], full["hit_ij"]) and same_bits(at["hit_stat"], full["hit_stat"])
    short = r_api.epistasis_host(G, y, min_stat=1.0, hit_cap=full["nhits"] - 1)
    assert short["nhits"] == full["nhits"] and short["ntested"] == full["ntested"] and short["max"] == full["max"]
    assert short["hit_ij"] is None and short["hit_stat"] is None and short["hit_mom"] is None
    allp = r_api.epistasis_host(G, y, min_stat=-math.inf)
    top = allp["hit_stat"].max()
    first = allp["hit_ij"][np.flatnonzero(allp["hit_stat"] == top)[0]]
    assert allp["max"] == (int(first[0]), int(first[1]), float(top))
    k2 = [k for k, (i, j) in enumerate(allp["hit_ij"].tolist()) if (i, j) == (0, 2)][0]
    k7 = [k for k, (i, j) in enumerate(allp["hit_ij"].tolist()) if (i, j) == (0, 7)][0]
    assert allp["hit_stat"][k2] == allp["hit_stat"][k7]
