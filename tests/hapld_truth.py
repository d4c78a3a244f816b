"""Truth for the pairwise haplotype EM and the haplotype blocks (include/eagle_hip.h section 1b''''vii), shared by tests/test_hapld_host.py
and tests/test_gpu_hapld.py.  Nothing here calls the feature: plain counting loops over individuals, a scalar Python loop of the rule
(Python floats are IEEE fp64, one rounding per operation), the same EM in mpmath at 40 digits, brute-force block partitions on sets of
pairs, and the panels the tests plant their structure in."""
import numpy as np


# ---- the 3 x 3 table by counting ----
def count_cells(gi, gj):
    """N[a][b] = the individuals with a B alleles at marker i and b at marker j (g + 1 = the number of B alleles)."""
    N = [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
    for a, b in zip(gi, gj):
        N[int(a) + 1][int(b) + 1] += 1
    return N


def pair_sums(gi, gj):
    """(s_i, q_i, s_j, q_j, d, e, f, h) by loops over the individuals."""
    si = qi = sj = qj = d = e = f = h = 0
    for a, b in zip(gi, gj):
        a, b = int(a), int(b)
        si += a; qi += a * a; sj += b; qj += b * b
        d += a * b; e += a * a * b * b; f += a * a * b; h += a * b * b
    return si, qi, sj, qj, d, e, f, h


# ---- the rule, one pair at a time ----
def scalar_rule(gi, gj, tol=1e-10, max_iter=1000, fg_cut=0.01, dprime_cut=0.8):
    """The header's rule for one pair from the counted table -> dict, or None for an undefined pair (a monomorphic member, n = 1)."""
    n = len(gi)
    N = count_cells(gi, gj)
    bi = 2 * sum(N[2]) + sum(N[1])
    bj = 2 * sum(r[2] for r in N) + sum(r[1] for r in N)
    if n < 2 or not 0 < bi < 2 * n or not 0 < bj < 2 * n:
        return None
    kBB = 2 * N[2][2] + N[2][1] + N[1][2]
    kBA = 2 * N[2][0] + N[2][1] + N[1][0]
    kAB = 2 * N[0][2] + N[0][1] + N[1][2]
    kAA = 2 * N[0][0] + N[0][1] + N[1][0]
    x = N[1][1]
    assert kBB + kBA + kAB + kAA + 2 * x == 2 * n
    T = float(2 * n)
    pi, qi, pj, qj = float(bi) / T, float(2 * n - bi) / T, float(bj) / T, float(2 * n - bj) / T
    pBB, pBA, pAB, pAA = pi * pj, pi * qj, qi * pj, qi * qj
    it = code = 0
    if x == 0:
        pBB, pBA, pAB, pAA = float(kBB) / T, float(kBA) / T, float(kAB) / T, float(kAA) / T
    else:
        while True:
            u = pBB * pAA
            v = pBA * pAB
            den = u + v
            t = u / den if den > 0.0 else 0.5
            xt = float(x) * t
            xo = float(x) - xt
            nBB = (float(kBB) + xt) / T
            delta = abs(nBB - pBB)
            pBB, pAA, pBA, pAB = nBB, (float(kAA) + xt) / T, (float(kBA) + xo) / T, (float(kAB) + xo) / T
            it += 1
            if delta <= tol:
                break
            if it == max_iter:
                code = 1
                break
    D = pBB - pi * pj
    dmax = min(pi * qj, qi * pj) if D >= 0.0 else min(pi * pj, qi * qj)
    dprime = max(-1.0, min(1.0, D / dmax))
    r2 = (D * D) / ((pi * qi) * (pj * qj))
    pmin = min(pBB, pBA, pAB, pAA)
    return {"pBB": pBB, "dprime": dprime, "r2": r2, "pmin": pmin, "iterations": it, "code": code, "recomb": pmin > fg_cut,
            "strong": abs(dprime) >= dprime_cut, "x": x, "k": (kBB, kBA, kAB, kAA)}


def mp_fixed_point(gi, gj, cap=6000):
    """The same EM in mpmath at 40 digits to delta <= 1e-30 -> dict with pBB, D, dmax candidates, dprime, r2 as mpf and rho, the ratio
    of the last two steps (0.0 without an iteration or where the last step is 0; 1.0 where the cap was hit)."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 40
    n = len(gi)
    N = count_cells(gi, gj)
    bi = 2 * sum(N[2]) + sum(N[1])
    bj = 2 * sum(r[2] for r in N) + sum(r[1] for r in N)
    k = [mp.mpf(v) for v in (2 * N[2][2] + N[2][1] + N[1][2], 2 * N[2][0] + N[2][1] + N[1][0], 2 * N[0][2] + N[0][1] + N[1][2],
                             2 * N[0][0] + N[0][1] + N[1][0])]
    x, T = mp.mpf(N[1][1]), mp.mpf(2 * n)
    pi, qi, pj, qj = mp.mpf(bi) / T, mp.mpf(2 * n - bi) / T, mp.mpf(bj) / T, mp.mpf(2 * n - bj) / T
    pBB, pBA, pAB, pAA = pi * pj, pi * qj, qi * pj, qi * qj
    rho = 0.0
    if N[1][1] == 0:
        pBB = k[0] / T
    else:
        prev = None
        stop = mp.mpf(10) ** -30
        for it in range(cap):
            u, v = pBB * pAA, pBA * pAB
            den = u + v
            t = u / den if den > 0 else mp.mpf(1) / 2
            xt = x * t
            xo = x - xt
            nBB = (k[0] + xt) / T
            delta = abs(nBB - pBB)
            pBB, pAA, pBA, pAB = nBB, (k[3] + xt) / T, (k[1] + xo) / T, (k[2] + xo) / T
            if delta <= stop:
                rho = float(delta / prev) if prev else 0.0
                break
            prev = delta
        else:
            rho = 1.0
    D = pBB - pi * pj
    d_pos, d_neg = min(pi * qj, qi * pj), min(pi * pj, qi * qj)
    dmax = d_pos if D >= 0 else d_neg
    den = (pi * qi) * (pj * qj)
    return {"pBB": pBB, "D": D, "dmax": dmax, "dmax_least": min(d_pos, d_neg), "dprime": max(-1, min(1, D / dmax)), "r2": D * D / den,
            "den": den, "rho": rho}


# ---- masks and brute-force blocks ----
def bit(mask, i, j):
    o = j - i
    return bool((int(mask[i, (o - 1) // 64]) >> ((o - 1) % 64)) & 1)


def mask_from_pairs(pairs, L, window):
    m = np.zeros((L, (window + 63) // 64), dtype=np.uint64)
    for i, j in pairs:
        assert 0 <= i < j < L and j - i <= window
        m[i, (j - i - 1) // 64] |= np.uint64(1) << np.uint64((j - i - 1) % 64)
    return m


def blocks_brute(recomb, strong, L, window, chrom=None, pos=None, kb=None, method="fourgamete", min_snp=2):
    """The block definition on SETS of pairs (i, j), i < j, by plain loops -> list of (first, last)."""
    def reach(i, j):
        if j - i > window:
            return False
        if chrom is not None and chrom[i] != chrom[j]:
            return False
        return kb is None or abs(int(pos[j]) - int(pos[i])) <= int(round(kb * 1000))

    out, i = [], 0
    while i < L:
        if method == "fourgamete":
            j = i
            while j + 1 < L and reach(i, j + 1) and not any((k, j + 1) in recomb for k in range(i, j + 1)):
                j += 1
        else:
            j = i
            for cand in range(i + 1, L):
                if not reach(i, cand):
                    break
                if all((i, k) in strong for k in range(i + 1, cand + 1)) and all((k, cand) in strong for k in range(i, cand)):
                    j = cand                                      # the largest such cand wins
        if j - i + 1 >= min_snp:
            out.append((i, j))
        i = j + 1
    return out


# ---- panels ----
def partner_panel(n, L, seed):
    """Random genotypes with what the shapes allow: identical and negated markers across the 128-marker tile edge (127 | 128) and the
    32-row block edge (31 | 32 | 33), monomorphic markers beside those edges."""
    from eagleeverything_amd import synth
    Mt8 = synth.genotypes_marker_major(n, L, seed=seed)
    if L >= 129:
        Mt8[127] = Mt8[124]
        Mt8[128] = -Mt8[124]
        Mt8[126] = 1
        Mt8[31] = Mt8[32]
        Mt8[33] = -Mt8[32]
        Mt8[30] = -1
    if L >= 300:
        Mt8[255] = Mt8[256] = Mt8[258]
        Mt8[257] = -1
        Mt8[299] = -Mt8[297]
    return Mt8


def founder_mosaic(n, L, founders=6, switch=0.03, seed=3):
    """Unphased genotypes (L, n) int8 of individuals whose two haplotypes are mosaics of a few founder haplotypes."""
    rng = np.random.default_rng(seed)
    F = (rng.random((founders, L)) < rng.uniform(0.2, 0.8, L)).astype(np.int8)
    hap = np.empty((2 * n, L), dtype=np.int8)
    for a in range(2 * n):
        src = rng.integers(founders)
        for m in range(L):
            if rng.random() < switch:
                src = rng.integers(founders)
            hap[a, m] = F[src, m]
    return np.ascontiguousarray((hap[0::2] + hap[1::2] - 1).T.astype(np.int8))


def planted_blocks(n=300, sizes=(5, 20, 7, 12, 9, 20, 5, 16) * 4, seed=11):
    """Blocks of 5 to 20 markers that each carry only three of the four gametes, independent of each other -> (Mt8 (L, n) int8,
    [(first, last)]).  Inside a block of m markers haplotype type t, 0 <= t <= m, has allele B at the markers below t: for a < b the
    gamete (A at a, B at b) does not exist.  Types 0 and m have frequency 0.3 each, so the last marker of a block (B in type m alone) and
    the first of the next (A in type 0 alone) show all four gametes at about 0.09 or more."""
    rng = np.random.default_rng(seed)
    cols, bounds, at = [], [], 0
    for m in sizes:
        w = np.full(m + 1, 0.4 / (m - 1))
        w[0] = w[m] = 0.3
        t = rng.choice(m + 1, size=2 * n, p=w)
        hap = (np.arange(m)[None, :] < t[:, None]).astype(np.int8)          # (2n, m)
        cols.append(hap[0::2] + hap[1::2] - 1)
        bounds.append((at, at + m - 1))
        at += m
    return np.ascontiguousarray(np.concatenate(cols, axis=1).T.astype(np.int8)), bounds
