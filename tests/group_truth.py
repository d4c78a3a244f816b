"""Truth for the per-group counts and the statistics made of them (include/eagle_hip.h section 1b''''iii), sharing no code with the
feature: pure-Python loops over individuals for the counts, and exact rational arithmetic (fractions.Fraction) for Hudson's and
Weir-Cockerham's Fst, the five case/control chi-squares and the Fisher tail.  No numpy arithmetic and no floating point in here."""
from fractions import Fraction
from math import comb


# ---- counts: loops over individuals ----
def counts_loops(Mt8, labels, K):
    """Mt8[m][i] in {-1, 0, +1}, labels[i] in [-1, K) -> list L x K x 3 of the numbers of -1 / 0 / +1 per marker and group."""
    out = []
    for row in Mt8:
        c = [[0, 0, 0] for _ in range(K)]
        for g, k in zip(row, labels):
            if k >= 0:
                c[int(k)][int(g) + 1] += 1
        out.append(c)
    return out


def bed_counts_loops(codes, labels, K):
    """codes[m][i] the 2-bit .bed codes (0 hom A1, 1 missing, 2 het, 3 hom A2) -> list L x K x 4 = (hom A1, het, hom A2, missing)."""
    col = {0: 0, 2: 1, 3: 2, 1: 3}
    out = []
    for row in codes:
        c = [[0, 0, 0, 0] for _ in range(K)]
        for v, k in zip(row, labels):
            if k >= 0:
                c[int(k)][col[int(v)]] += 1
        out.append(c)
    return out


# ---- Fst ----
def hudson(c1, c2):
    """(num, den) of Hudson's estimator (Bhatia et al. 2013) for two groups' called counts (n0, n1, n2), as Fractions; None when a group has
    fewer than 2 called individuals or den = 0.  Also the condition number of num: the sum of |terms| over |num| (None if num = 0)."""
    (a0, a1, a2), (b0, b1, b2) = [tuple(int(v) for v in c[:3]) for c in (c1, c2)]
    na, nb = a0 + a1 + a2, b0 + b1 + b2
    if na < 2 or nb < 2:
        return None
    p1, p2 = Fraction(2 * a2 + a1, 2 * na), Fraction(2 * b2 + b1, 2 * nb)
    terms = [(p1 - p2) ** 2, -p1 * (1 - p1) / (2 * na - 1), -p2 * (1 - p2) / (2 * nb - 1)]
    num, den = sum(terms), p1 * (1 - p2) + p2 * (1 - p1)
    if den == 0:
        return None
    return num, den, (sum(abs(t) for t in terms) / abs(num) if num != 0 else None)


def weir_cockerham(groups):
    """(a, b, c) of Weir and Cockerham (1984) over r groups' called counts (n0, n1, n2), as Fractions; None when a group has fewer than 2
    called individuals or n_c = 0 or a + b + c = 0."""
    r = len(groups)
    n = [int(g[0]) + int(g[1]) + int(g[2]) for g in groups]
    if min(n) < 2:
        return None
    p = [Fraction(2 * int(g[2]) + int(g[1]), 2 * ni) for g, ni in zip(groups, n)]
    h = [Fraction(int(g[1]), ni) for g, ni in zip(groups, n)]
    nbar = Fraction(sum(n), r)
    nc = (r * nbar - Fraction(sum(ni * ni for ni in n), 1) / (r * nbar)) / (r - 1)
    pbar = sum(ni * pi for ni, pi in zip(n, p)) / (r * nbar)
    s2 = sum(ni * (pi - pbar) ** 2 for ni, pi in zip(n, p)) / ((r - 1) * nbar)
    hbar = sum(ni * hi for ni, hi in zip(n, h)) / (r * nbar)
    if nc == 0:
        return None
    a = (nbar / nc) * (s2 - (pbar * (1 - pbar) - Fraction(r - 1, r) * s2 - hbar / 4) / (nbar - 1))
    b = (nbar / (nbar - 1)) * (pbar * (1 - pbar) - Fraction(r - 1, r) * s2 - ((2 * nbar - 1) / (4 * nbar)) * hbar)
    c = hbar / 2
    if a + b + c == 0:
        return None
    return a, b, c


# ---- case/control ----
def pearson(table):
    """Pearson's chi-square of an r x c table of ints as a Fraction; None with a zero margin."""
    rows = [sum(r) for r in table]
    cols = [sum(r[j] for r in table) for j in range(len(table[0]))]
    N = sum(rows)
    if 0 in rows or 0 in cols:
        return None
    return sum(Fraction(table[i][j] - Fraction(rows[i] * cols[j], N)) ** 2 / Fraction(rows[i] * cols[j], N)
               for i in range(len(table)) for j in range(len(cols)))


def case_control(cases, controls):
    """The five statistics of a marker from the called counts (r0, r1, r2) of the cases and (s0, s1, s2) of the controls, as Fractions
    (None with a zero margin): allelic, trend (Cochran-Armitage, weights 0 1 2), genotypic, dominant, recessive; and the allele table."""
    r0, r1, r2 = (int(v) for v in cases[:3])
    s0, s1, s2 = (int(v) for v in controls[:3])
    allele = (2 * r2 + r1, 2 * r0 + r1, 2 * s2 + s1, 2 * s0 + s1)
    R, S = r0 + r1 + r2, s0 + s1 + s2
    N, n1, n2 = R + S, r1 + s1, r2 + s2
    var = N * (n1 + 4 * n2) - (n1 + 2 * n2) ** 2
    trend = None if R == 0 or S == 0 or var == 0 else Fraction(N * (N * (r1 + 2 * r2) - R * (n1 + 2 * n2)) ** 2, R * S * var)
    return {"allelic": pearson([allele[:2], allele[2:]]), "trend": trend, "genotypic": pearson([[r0, r1, r2], [s0, s1, s2]]),
            "dominant": pearson([[r1 + r2, r0], [s1 + s2, s0]]), "recessive": pearson([[r2, r0 + r1], [s2, s0 + s1]]), "allele": allele}


# ---- Fisher ----
FISHER_SLACK = Fraction(10000001, 10000000)     # 1 + 10^-7, the rule of R's fisher.test


def fisher(a, b, c, d):
    """(p, gap): the two-sided exact p of (a, b; c, d) -- the sum of the hypergeometric terms with P(x) <= P(a) (1 + 10^-7) -- as a
    Fraction, and gap = min over x of |P(x) / P(a) - (1 + 10^-7)|: how far the nearest term lies from the rule's edge."""
    r1, r2, c1 = a + b, c + d, a + c
    if r1 + r2 == 0:
        return Fraction(1), None
    lo, hi = max(0, c1 - r2), min(r1, c1)
    w = {x: comb(r1, x) * comb(r2, c1 - x) for x in range(lo, hi + 1)}
    cut = w[a] * FISHER_SLACK
    p = Fraction(sum(v for v in w.values() if v <= cut), sum(w.values()))
    gap = min(abs(Fraction(v, w[a]) - FISHER_SLACK) for v in w.values())
    return p, gap


# The 2 x 2 tables (a, b, c, d) the host and the device Fisher tests share: every margin <= 1,000; balanced designs (r1 = r2) whose terms x
# and c1 - x are mathematically tied; zero cells; lopsided margins.  test_groups_host asserts that no term of any of them lies within
# 10^-9 of the rule's edge P(a) (1 + 10^-7), so the exact tail and an fp64 walk select the same terms.
FISHER_TABLES = [
    (3, 1, 1, 3), (1, 3, 3, 1), (5, 5, 5, 5), (10, 0, 0, 10), (0, 10, 10, 0), (7, 3, 2, 8), (2, 8, 7, 3), (12, 8, 8, 12), (8, 12, 12, 8),
    (1, 0, 0, 1), (1, 0, 0, 0), (0, 0, 0, 7), (0, 5, 0, 9), (4, 0, 6, 0), (20, 30, 30, 20), (30, 20, 20, 30), (25, 25, 20, 30),
    (100, 100, 80, 120), (120, 80, 100, 100), (100, 100, 100, 100), (150, 50, 50, 150), (50, 150, 150, 50), (300, 0, 0, 300),
    (250, 250, 200, 300), (200, 300, 250, 250), (499, 1, 1, 499), (1, 499, 499, 1), (500, 500, 0, 0), (17, 483, 2, 498), (2, 498, 17, 483),
    (333, 167, 201, 299), (400, 100, 350, 150), (1, 499, 0, 500), (13, 7, 480, 500), (250, 250, 250, 250), (260, 240, 240, 260),
    (240, 260, 260, 240), (37, 41, 43, 47), (6, 494, 9, 491), (9, 491, 6, 494), (450, 50, 50, 450),
]
