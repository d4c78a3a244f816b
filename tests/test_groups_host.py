"""CPU: the numpy restatements of the per-group counts and the statistics on top (r_api.group_counts_host, bed_group_counts_host,
fisher_2x2_host, fst_from_counts, case_control_from_counts) against tests/group_truth.py: loops over individuals and exact rational
arithmetic.  Counts are compared with ==.

Tolerances.  The statistics form every integer part exactly (int64) and then apply at most ~25 correctly rounded fp64 operations.  A
subtraction of fp64 values amplifies the relative error carried into it by cond = (sum of |terms|) / |result|; the markers used below are
CHOSEN, in exact arithmetic, so that every such subtraction has cond <= 4 and every sum across markers adds positive numbers only.  The
deepest chain (F_IS: the b bracket, then 1 - c / (b + c)) nests two subtractions: 25 * 16 * 2^-53 = 4.4e-14 < 1e-13, the relative
tolerance.  fisher_2x2_host: at most 1,000 recurrence steps of two roundings each plus the sums of positive terms, about 3 * 1000 * 2^-53
= 3.4e-13 < 1e-12 relative, on tables with margins <= 1,000."""
from fractions import Fraction

import numpy as np
import pytest

import group_truth as truth

REL = 1e-13
FISHER_REL = 1e-12


def close(got, exact, rel):
    """|got - exact| <= rel |exact|, decided in exact arithmetic."""
    return abs(Fraction(np.asarray(got).item()) - exact) <= Fraction(rel) * abs(exact)


def panel(L, n, seed, K, unlabelled=0.1):
    rng = np.random.default_rng(seed)
    Mt8 = rng.integers(-1, 2, (L, n)).astype(np.int8)
    labels = rng.integers(0, K, n)
    labels[rng.random(n) < unlabelled] = -1
    return Mt8, labels.astype(np.int32)


# ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("L,n,K", [(5, 1, 1), (7, 33, 3), (9, 130, 64), (4, 257, 33)])
def test_restatements_equal_the_loops(L, n, K):
    from eagleeverything_amd import r_api
    Mt8, labels = panel(L, n, 10 * L + n, K)
    if K > 2:
        labels[labels == 1] = -1                                    # an empty group
    got = r_api.group_counts_host(Mt8, labels, K)
    assert got.dtype == np.int32 and got.shape == (L, K, 3)
    assert got.tolist() == truth.counts_loops(Mt8.tolist(), labels.tolist(), K)
    codes = np.random.default_rng(n).integers(0, 4, (L, n)).astype(np.uint8)
    got = r_api.bed_group_counts_host(codes, labels, K)
    assert got.dtype == np.int32 and got.shape == (L, K, 4)
    assert got.tolist() == truth.bed_counts_loops(codes.tolist(), labels.tolist(), K)
    assert not r_api.group_counts_host(Mt8, np.full(n, -1), K).any()


def test_sum_over_groups_is_marker_stats_counts():
    from eagleeverything_amd import r_api
    Mt8, labels = panel(40, 203, 5, 7, unlabelled=0.0)
    c = r_api.group_counts_host(Mt8, labels, 7)
    whole = np.stack([np.sum(Mt8 == v, axis=1) for v in (-1, 0, 1)], axis=1)
    assert np.array_equal(c.sum(axis=1), whole)
    assert np.array_equal(r_api.group_counts_host(Mt8, np.zeros(203, dtype=np.int32), 1)[:, 0], whole)      # K = 1 is marker_counts
    a, b = r_api.marker_stats_from_counts(*c.sum(axis=1).T), r_api.marker_stats_from_counts(*whole.T)
    assert all(np.array_equal(a[k], b[k]) for k in b)
    codes = np.random.default_rng(1).integers(0, 4, (40, 203)).astype(np.uint8)
    cb = r_api.bed_group_counts_host(codes, labels, 7)
    assert np.array_equal(cb.sum(axis=1), np.stack([np.sum(codes == v, axis=1) for v in (0, 2, 3, 1)], axis=1))


def test_group_labels():
    from eagleeverything_amd import r_api
    lab, names = r_api.group_labels(["b", None, "a", float("nan"), "b", "c"])
    assert lab.dtype == np.int32 and lab.tolist() == [1, -1, 0, -1, 1, 2] and names == ["a", "b", "c"]
    lab, names = r_api.group_labels(np.array([2.0, np.nan, 0.0, 2.0]))
    assert lab.tolist() == [1, -1, 0, 1] and names == [0.0, 2.0]


# ------------------------------------------------------------------------------------------------ planted values
def test_planted_fst_values():
    from eagleeverything_amd import r_api
    fixed = np.array([[[30, 0, 0], [0, 0, 41]], [[0, 0, 30], [41, 0, 0]]])       # two groups fixed for opposite alleles
    h = r_api.fst_from_counts(fixed)
    assert h["fst"].tolist() == [[1.0], [1.0]] and h["genome"].tolist() == [1.0] and h["matrix"].tolist() == [[0.0, 1.0], [1.0, 0.0]]
    w = r_api.fst_from_counts(fixed, method="wc")
    assert all(close(t, Fraction(1), REL) for t in w["theta"]) and close(w["genome"], Fraction(1), REL)     # b = c = 0 in exact arithmetic
    halves = np.array([[[12, 20, 8], [12, 20, 8]]])                             # one group split in two identical halves
    num, den, _ = truth.hudson(halves[0, 0], halves[0, 1])
    assert num < 0 and num == -2 * Fraction(9, 20) * Fraction(11, 20) / 79
    h = r_api.fst_from_counts(halves)
    assert close(h["num"][0, 0], num, REL) and close(h["den"][0, 0], den, REL) and close(h["fst"][0, 0], num / den, REL)
    a, b, c = truth.weir_cockerham(halves[0])
    w = r_api.fst_from_counts(halves, method="wc")
    assert a < 0 and close(w["theta"][0], a / (a + b + c), REL) and close(w["c"][0], c, REL)
    # fewer than 2 called individuals in a group, and a marker monomorphic everywhere (den = 0): NaN, left out of the sums
    odd = np.array([[[12, 20, 8], [1, 0, 0]], [[40, 0, 0], [35, 0, 0]], [[30, 0, 0], [0, 0, 41]]])
    for method, key in (("hudson", "fst"), ("wc", "theta")):
        r = r_api.fst_from_counts(odd, method=method)
        assert np.isnan(r[key][:2]).all() and close(r[key][2], Fraction(1), REL) and close(np.ravel(r["genome"])[0], Fraction(1), REL)


def test_planted_trend_table():
    from eagleeverything_amd import r_api
    # cases (10, 20, 30), controls (30, 20, 10): N = 120, N (r1 + 2 r2) - R (n1 + 2 n2) = 9600 - 7200 = 2400, the variance term
    # 120 * 200 - 120^2 = 9600, so the trend chi-square is 120 * 2400^2 / (60 * 60 * 9600) = 20
    cc = r_api.case_control_from_counts(np.array([[[30, 20, 10], [10, 20, 30]]]))
    assert truth.case_control((10, 20, 30), (30, 20, 10))["trend"] == 20
    assert cc["trend"].tolist() == [20.0] and cc["cases"].tolist() == [[10, 20, 30]] and cc["controls"].tolist() == [[30, 20, 10]]
    assert cc["or"].tolist() == [(80 * 80) / (40 * 40)]
    from scipy import special
    assert cc["p_trend"].tolist() == [special.chdtrc(1.0, 20.0)] and cc["p_genotypic"][0] == special.chdtrc(2.0, cc["genotypic"][0])
    zero = r_api.case_control_from_counts(np.array([[[0, 0, 0], [10, 20, 30]], [[5, 5, 0], [6, 4, 0]]]))    # no controls; nobody '2'
    assert np.isnan(zero["allelic"][0]) and np.isnan(zero["trend"][0]) and np.isnan(zero["genotypic"]).all() and np.isnan(zero["recessive"][1])
    assert not np.isnan(zero["allelic"][1]) and not np.isnan(zero["dominant"][1])


# ------------------------------------------------------------------------------------------------ statistics against Fraction
def structured_counts(seed, r, L=150):
    """Called genotype counts (L, r, 3) of r inbred populations (F = 0.6) with allele frequencies spread over [0.25, 0.75]: far from
    Hardy-Weinberg inside a group and far apart between groups, so that no variance component is a difference of near-equal numbers."""
    rng = np.random.default_rng(seed)
    sizes = [40, 53, 47, 61][:r]
    out = np.zeros((L, r, 3), dtype=np.int64)
    for m in range(L):
        ps = np.linspace(0.25, 0.75, r) + rng.uniform(-0.05, 0.05, r)
        for k in range(r):
            p, F = ps[k], 0.6
            out[m, k] = rng.multinomial(sizes[k], [(1 - p) ** 2 + F * p * (1 - p), 2 * p * (1 - p) * (1 - F), p * p + F * p * (1 - p)])
    return out


def cond(terms):
    return sum(abs(t) for t in terms) / abs(sum(terms))


def wc_well_conditioned(groups):
    """Every subtraction of the Weir-Cockerham formulas, in exact arithmetic, has cond <= 4, and a, b, c are positive."""
    r = len(groups)
    n = [int(sum(g)) for g in groups]
    p = [Fraction(int(2 * g[2] + g[1]), 2 * ni) for g, ni in zip(groups, n)]
    nbar = Fraction(sum(n), r)
    pbar = sum(ni * pi for ni, pi in zip(n, p)) / (r * nbar)
    s2 = sum(ni * (pi - pbar) ** 2 for ni, pi in zip(n, p)) / ((r - 1) * nbar)
    hbar = Fraction(int(sum(g[1] for g in groups))) / (r * nbar)
    pq, rr = pbar * (1 - pbar), Fraction(r - 1, r)
    inner = [pq, -rr * s2, -hbar / 4]
    abc = truth.weir_cockerham(groups)
    if abc is None or min(abc) <= 0 or sum(inner) == 0:
        return False
    a, b, c = abc
    return max(cond(inner), cond([s2, -sum(inner) / (nbar - 1)]), cond([pq, -rr * s2, -((2 * nbar - 1) / (4 * nbar)) * hbar]),
               cond([Fraction(1), -c / (b + c)]), cond([nbar * r, -Fraction(sum(ni * ni for ni in n)) / (r * nbar)])) <= 4


@pytest.mark.parametrize("r", [2, 4])
def test_fst_against_fractions(r):
    from eagleeverything_amd import r_api
    counts = structured_counts(3 + r, r)
    # the markers chosen: every subtraction well conditioned (module docstring), for Hudson's numerator of every pair too
    keep = [m for m in range(len(counts)) if wc_well_conditioned(counts[m]) and
            all(truth.hudson(counts[m, i], counts[m, j])[2] <= 4 and truth.hudson(counts[m, i], counts[m, j])[0] > 0
                for i in range(r) for j in range(i + 1, r))]
    assert len(keep) >= 30
    counts = counts[keep]
    h = r_api.fst_from_counts(counts)
    assert h["pairs"].tolist() == [[i, j] for i in range(r) for j in range(i + 1, r)] and h["fst"].shape == (len(keep), r * (r - 1) // 2)
    for t, (i, j) in enumerate(h["pairs"]):
        ex = [truth.hudson(counts[m, i], counts[m, j]) for m in range(len(keep))]
        assert all(close(h["fst"][m, t], e[0] / e[1], REL) for m, e in enumerate(ex))
        genome = sum(e[0] for e in ex) / sum(e[1] for e in ex)
        assert close(h["genome"][t], genome, REL) and h["matrix"][i, j] == h["genome"][t] == h["matrix"][j, i]
    w = r_api.fst_from_counts(counts, method="wc")
    ex = [truth.weir_cockerham(counts[m]) for m in range(len(keep))]
    for m, (a, b, c) in enumerate(ex):
        assert close(w["a"][m], a, REL) and close(w["b"][m], b, REL) and close(w["c"][m], c, REL)
        assert close(w["theta"][m], a / (a + b + c), REL) and close(w["fis"][m], 1 - c / (b + c), REL)
    A, B, Cc = (sum(e[k] for e in ex) for k in range(3))
    assert close(w["genome"], A / (A + B + Cc), REL) and close(w["genome_fis"], 1 - Cc / (B + Cc), REL)


def test_fst_windows_cut_at_chromosome_ends():
    from eagleeverything_amd import r_api
    counts = structured_counts(11, 2, L=23)
    chrom = np.array([0] * 10 + [1] * 13)
    pos = np.r_[np.arange(10) * 700 + 100, np.arange(13) * 400 + 50]
    h = r_api.fst_from_counts(counts, chrom=chrom, window=4)
    assert h["windows"]["first"].tolist() == [0, 4, 8, 10, 14, 18, 22] and h["windows"]["last"].tolist() == [3, 7, 9, 13, 17, 21, 22]
    assert h["windows"]["chrom"].tolist() == [0, 0, 0, 1, 1, 1, 1]
    for wdw, (f, l) in enumerate(zip(h["windows"]["first"], h["windows"]["last"])):
        ex = [truth.hudson(counts[m, 0], counts[m, 1]) for m in range(f, l + 1)]
        assert all(e[0] > 0 for e in ex) and close(h["windows"]["fst"][wdw, 0], sum(e[0] for e in ex) / sum(e[1] for e in ex), REL)
    k = r_api.fst_from_counts(counts, method="wc", chrom=chrom, pos=pos, kb=2.0)
    cells = [(c, p // 2000) for c, p in zip(chrom.tolist(), pos.tolist())]
    firsts = [i for i in range(23) if i == 0 or cells[i] != cells[i - 1]]
    assert k["windows"]["first"].tolist() == firsts and len(k["windows"]["theta"]) == len(firsts)
    with pytest.raises(ValueError):
        r_api.fst_from_counts(counts, kb=2.0)


def test_case_control_against_fractions():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(8)
    counts = np.zeros((50, 2, 3), dtype=np.int64)
    for m in range(50):
        p = rng.uniform(0.2, 0.8)
        counts[m, 0] = rng.multinomial(157, [(1 - p) ** 2, 2 * p * (1 - p), p * p])
        q = min(0.9, p + rng.uniform(0.0, 0.2))
        counts[m, 1] = rng.multinomial(131, [(1 - q) ** 2, 2 * q * (1 - q), q * q])
    counts[0] = [[157, 0, 0], [131, 0, 0]]                                      # a zero margin everywhere
    cc = r_api.case_control_from_counts(counts)
    # Every statistic is N * (an exact integer)^2 over a product of exact integers, or a sum of six such positive terms: no fp64
    # subtraction at all, and the denominators are exact non-zero integers (asserted by the truth returning a value).
    for m in range(50):
        ex = truth.case_control(counts[m, 1], counts[m, 0])
        for key in ("allelic", "trend", "genotypic", "dominant", "recessive"):
            if ex[key] is None:
                assert m == 0 and np.isnan(cc[key][m]) and np.isnan(cc["p_" + key][m])
            else:
                assert close(cc[key][m], ex[key], REL), (m, key)
        a, b, c, d = ex["allele"]
        if b * c:
            assert close(cc["or"][m], Fraction(a * d, b * c), REL)
    assert cc["cases"].tolist() == counts[:, 1].tolist() and cc["controls"].tolist() == counts[:, 0].tolist()
    four = np.concatenate([counts, np.full((50, 2, 1), 9)], axis=2)             # the missing column of the .bed route is not used
    cf = r_api.case_control_from_counts(four)
    assert all(np.array_equal(cf[k], cc[k], equal_nan=True) for k in cc)


# ------------------------------------------------------------------------------------------------ Fisher
def test_fisher_tables_are_clear_of_the_edge():
    """No exact ratio P(x) / P(a) of the shared tables lies within 1e-9 of 1 + 1e-7; the balanced ones do hold exact ties."""
    tied = 0
    for a, b, c, d in truth.FISHER_TABLES:
        assert min(a, b, c, d) >= 0 and max(a + b, c + d, a + c, b + d) <= 1000
        p, gap = truth.fisher(a, b, c, d)
        assert gap is None or gap >= Fraction(1, 10 ** 9), (a, b, c, d)
        tied += a + b == c + d and (a + c) - a != a and a + b > 0               # x = a and x = c1 - a are two terms of equal weight
    assert tied >= 10


def test_fisher_host_against_fractions():
    from eagleeverything_amd import r_api
    got = r_api.fisher_2x2_host(truth.FISHER_TABLES)
    assert got.dtype == np.float64 and got.shape == (len(truth.FISHER_TABLES),)
    for t, g in zip(truth.FISHER_TABLES, got):
        assert 0.0 < g <= 1.0 and close(g, truth.fisher(*t)[0], FISHER_REL), t
    known = dict(zip(truth.FISHER_TABLES, got))
    assert known[(0, 0, 0, 7)] == 1.0 and known[(500, 500, 0, 0)] == 1.0 and known[(5, 5, 5, 5)] == 1.0 and known[(1, 0, 0, 0)] == 1.0
    assert close(known[(3, 1, 1, 3)], Fraction(34, 70), FISHER_REL)             # (1 + 16 + 16 + 1) / C(8, 4)
    assert r_api.fisher_2x2_host([[0, 0, 0, 0]]).tolist() == [1.0]
    # a table and its mirror images select the same terms
    assert known[(7, 3, 2, 8)] == pytest.approx(known[(2, 8, 7, 3)], rel=FISHER_REL)
