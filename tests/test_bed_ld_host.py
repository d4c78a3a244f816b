"""CPU: the numpy restatements of pairwise-complete LD from a .bed file (r_api.bed_ld_host, bed_ld_mask_host, bed_ld_partners_host;
include/eagle_hip.h section 1b'''iv) against a plain double loop in Python ints and Fractions, against the panel's LD where the file has
no missing code, and what they are for: a missing call no longer pulls r2 towards the heterozygote.  No device work.

Concordance of LD-kNNi (k = 5, l = 16, window 50, local_min_overlap 4) on the founder-mosaic panel of tests/test_ldknn_host.py with the
partners ranked on the ingested panel / on the .bed file's pairwise-complete r2 (min_overlap 9), as printed by the last test:
    5 % masked:   seed 0  0.7955 / 0.7970    seed 1  0.7905 / 0.7930    seed 2  0.7948 / 0.8012
    20 % masked:  seed 0  0.7523 / 0.7617    seed 1  0.7410 / 0.7522    seed 2  0.7448 / 0.7491
The file's own r2 is ahead in all six, by 0.2 to 0.6 points at 5 % and 0.4 to 1.1 points at 20 %: too little room over three seeds to
assert an inequality, so only what the definition guarantees is asserted -- the same partners when nothing is masked."""
import functools
from fractions import Fraction

import numpy as np
import pytest

from test_ldknn_host import mosaic_panel, unpack

XVAL = {0: -1, 1: 0, 2: 0, 3: 1}


# ---- the definition as a plain double loop ----
def loop_pair(ci, cj, min_overlap):
    """(N, D, Si, Sj, Qi, Qj, comparable, cov, vi, vj) of two rows of codes, in Python ints."""
    N = D = Si = Sj = Qi = Qj = 0
    for a, b in zip(ci, cj):
        a, b = int(a), int(b)
        xa, xb, ca, cb = XVAL[a], XVAL[b], int(a != 1), int(b != 1)
        N += ca * cb
        D += xa * xb
        Si += xa * cb
        Sj += ca * xb
        Qi += abs(xa) * cb
        Qj += ca * abs(xb)
    cov, vi, vj = N * D - Si * Sj, N * Qi - Si * Si, N * Qj - Sj * Sj
    return N, D, Si, Sj, Qi, Qj, (N >= min_overlap and vi > 0 and vj > 0), cov, vi, vj


def fl(x):
    return float(Fraction(x))            # float(Fraction) is the correctly rounded value


def loop_band(codes, window, min_overlap, t):
    L = codes.shape[0]
    sums = np.zeros((6, L, window), dtype=np.int64)
    r2 = np.full((L, window), -1.0)
    bits = np.zeros((L, (window + 63) // 64 * 64), dtype=np.uint8)
    for i in range(L):
        for o in range(1, window + 1):
            if i + o >= L:
                continue
            N, D, Si, Sj, Qi, Qj, ok, cov, vi, vj = loop_pair(codes[i], codes[i + o], min_overlap)
            sums[:, i, o - 1] = (N, D, Si, Sj, Qi, Qj)
            if ok:
                num, den = fl(Fraction(cov) ** 2), fl(Fraction(vi) * Fraction(vj))
                r2[i, o - 1] = fl(Fraction(num) / Fraction(den))
                bits[i, o - 1] = num > fl(Fraction(t) * Fraction(den))
    return sums, r2, np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").astype(np.uint64)


@functools.lru_cache(maxsize=None)
def loop_panel():
    rng = np.random.default_rng(3)
    n, L = 23, 40
    codes = np.array([0, 2, 3], dtype=np.uint8)[rng.integers(0, 3, size=(L, n))]
    codes[rng.random((L, n)) < 0.3] = 1
    codes[5, :] = 1                                     # no call at all
    codes[6, 1:] = 1                                    # a single call
    codes[11] = codes[10]                               # the same marker twice, with the same calls: r2 = 1
    codes[12] = np.array([3, 1, 2, 0], dtype=np.uint8)[codes[10]]   # its complement, with the same calls: r2 = 1, cov < 0
    codes.setflags(write=False)
    return codes


@pytest.mark.parametrize("window,min_overlap,t", [(1, 1, 0.2), (7, 1, 0.0), (7, 8, 0.2), (39, 12, 0.5), (64, 1, 1.0), (65, 3, 0.05)])
def test_bed_ld_host_equals_the_double_loop(window, min_overlap, t):
    from eagleeverything_amd import r_api
    codes = loop_panel()
    L = codes.shape[0]
    got = r_api.bed_ld_host(codes, window, None, min_overlap)
    sums, r2, mask = loop_band(codes, window, min_overlap, t)
    assert len(got) == 7 and all(a.dtype == np.int64 and a.shape == (L, window) for a in got[:6]) and got[6].dtype == np.float64
    for a, b in zip(got[:6], sums):
        assert np.array_equal(a, b)
    assert np.array_equal(got[6].view(np.uint64), r2.view(np.uint64))                       # the same bits
    got_mask = r_api.bed_ld_mask_host(codes, window, t, None, min_overlap)
    assert got_mask.dtype == np.uint64 and got_mask.shape == (L, (window + 63) // 64) and np.array_equal(got_mask, mask)
    assert (got[6][5] == -1.0).all() and (got[6][6] == -1.0).all()                          # nothing to compare with
    assert (got[6][[4], 0] == -1.0).all() and (got[6][3, 1:3] == -1.0).all()                # ... seen from the markers before them
    if min_overlap == 1:
        assert got[6][10, 0] == 1.0 and (window < 2 or got[6][10, 1] == 1.0)                # a copy and the complement
    assert ((got[6] == -1.0) | ((got[6] >= 0.0) & (got[6] <= 1.0))).all()
    assert (got[0] < min_overlap).any() or min_overlap == 1


def test_bed_ld_host_include_is_the_sub_panel():
    from eagleeverything_amd import r_api
    codes = loop_panel()
    L = codes.shape[0]
    inc = np.arange(L) % 3 != 1
    for include in (inc, np.flatnonzero(inc)):
        a, b = r_api.bed_ld_host(codes, 9, include, 2), r_api.bed_ld_host(codes[inc], 9, None, 2)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert np.array_equal(r_api.bed_ld_mask_host(codes, 9, 0.1, include, 2), r_api.bed_ld_mask_host(codes[inc], 9, 0.1, None, 2))
        pa, pb = r_api.bed_ld_partners_host(codes, 9, 5, 0.0, include, 2), r_api.bed_ld_partners_host(codes[inc], 9, 5, 0.0, None, 2)
        assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    for bad in (dict(window=0), dict(window=257), dict(min_overlap=0), dict(include=np.zeros(L, dtype=bool))):
        kw = dict(window=5, include=None, min_overlap=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            r_api.bed_ld_host(codes, kw["window"], kw["include"], kw["min_overlap"])
    with pytest.raises(ValueError):
        r_api.bed_ld_mask_host(codes, 5, 1.5)
    with pytest.raises(ValueError):
        r_api.bed_ld_partners_host(codes, 5, 33, 0.0)
    with pytest.raises(ValueError):
        r_api.bed_ld_partners_host(codes, 5, 4, 0.0, chrom=np.zeros(3))


# ---- no missing code: the panel's LD, bit for bit ----
def panel_mask(Mt8, window, t):
    """include/eagle_hip.h section 1b'' on the int8 image (L, n): what eagle_ld_window computes and LDPrune prunes on."""
    G = Mt8.astype(np.int64)
    L, n = G.shape
    s, q = G.sum(axis=1), (G * G).sum(axis=1)
    v = n * q - s * s
    bits = np.zeros((L, (window + 63) // 64 * 64), dtype=np.uint8)
    band = np.full((L, window), -1.0)
    for o in range(1, min(window, L - 1) + 1):
        d = (G[:-o] * G[o:]).sum(axis=1)
        c = (n * d - s[:-o] * s[o:]).astype(np.float64)
        vi, vj = v[:-o], v[o:]
        ok = (vi > 0) & (vj > 0)
        den = vi.astype(np.float64) * vj.astype(np.float64)
        bits[:-o, o - 1] = ok & (c * c > np.float64(t) * den)
        band[:-o, o - 1] = np.where(ok, (c * c) / np.where(ok, den, 1.0), -1.0)
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").astype(np.uint64), band


@pytest.mark.parametrize("window,l,t", [(50, 16, 0.2), (5, 32, 0.0), (256, 7, 0.02), (1, 1, 0.5)])
def test_without_a_missing_code_it_is_the_panels_ld(window, l, t):
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(8)
    n, L = 37, 90
    Mt8 = rng.integers(-1, 2, size=(L, n)).astype(np.int8)
    for j in range(1, L):
        if rng.random() < 0.5:
            Mt8[j] = np.where(rng.random(n) < 0.1, Mt8[j], Mt8[j - 1])
    Mt8[7], Mt8[61] = 1, 0                                                                    # monomorphic
    codes = np.array([0, 2, 3], dtype=np.uint8)[Mt8 + 1]
    chrom = np.where(np.arange(L) < 40, 2, 1)
    mask, band = panel_mask(Mt8, window, t)
    for mo in (1, n):
        assert np.array_equal(r_api.bed_ld_mask_host(codes, window, t, None, mo), mask)
        assert np.array_equal(r_api.bed_ld_host(codes, window, None, mo)[6].view(np.uint64), band.view(np.uint64))
        for ch, min_r2 in ((None, 0.0), (chrom, 0.0), (None, t)):
            got, want = r_api.bed_ld_partners_host(codes, window, l, min_r2, None, mo, ch), r_api.ld_partners_host(Mt8, window, l, min_r2, ch)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
    N, D, Si, Sj, Qi, Qj, _ = r_api.bed_ld_host(codes, min(window, L - 1), None, 1)
    o = min(window, L - 1)
    G = Mt8.astype(np.int64)
    assert (N[:-o] == n).all() and np.array_equal(Si[:-o, 0], G.sum(axis=1)[:-o]) and np.array_equal(Qj[:-1, 0], (G * G).sum(axis=1)[1:])
    assert (r_api.bed_ld_host(codes, window, None, n + 1)[6] == -1.0).all()                   # nobody has n + 1 individuals


# ---- the bias this removes ----
def test_missing_calls_no_longer_pull_r2_towards_the_heterozygote():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(17)
    n, L, window, m = 240, 12, 5, 0.2
    Mt8 = (2 * rng.integers(0, 2, size=(L, n)) - 1).astype(np.int8)                           # inbred lines: x = +-1
    Mt8[4] = Mt8[3]                                                                           # one marker twice
    miss = np.zeros((L, n), dtype=bool)
    miss[3], miss[4] = rng.random(n) < m, rng.random(n) < m                                   # 20 % of each copy, independently
    codes = np.array([0, 2, 3], dtype=np.uint8)[Mt8 + 1]
    codes[miss] = 1
    ingested = np.array([-1, 0, 0, 1], dtype=np.int8)[codes]                                  # missing = heterozygous
    panel, band = panel_mask(ingested, window, 0.9)
    r2_bed = r_api.bed_ld_host(codes, window)[6]
    print("r2 of the two copies: het-filled %.4f (expected near %.2f), pairwise-complete %r" % (band[3, 0], (1 - m) ** 2, r2_bed[3, 0]))
    assert band[3, 0] < 0.9
    assert r2_bed[3, 0] == 1.0
    bed = r_api.bed_ld_mask_host(codes, window, 0.9, None, max(2, n // 10))
    keep_bed, keep_panel = r_api.ld_prune_keep(bed, window), r_api.ld_prune_keep(panel, window)
    assert keep_panel.all()
    assert np.flatnonzero(~keep_bed).tolist() == [4]
    part, pr2 = r_api.bed_ld_partners_host(codes, window, 3, 0.0)
    assert part[3, 0] == 4 and part[4, 0] == 3 and pr2[3, 0] == 1.0


# ---- LD-kNNi with partners from the file ----
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ldknn_with_partners_from_the_bed_file_on_a_founder_mosaic(seed):
    from eagleeverything_amd import r_api
    k, l, window = 5, 16, 50
    for rate in (0.0, 0.05, 0.20):
        codes, truth, mask = mosaic_panel(seed, rate=rate)
        L, n = codes.shape
        mo = max(2, n // 10)
        Mt8 = np.array([-1, 0, 0, 1], dtype=np.int8)[codes]
        p_panel, r_panel = r_api.ld_partners_host(Mt8, window, l, 0.0)
        p_bed, r_bed = r_api.bed_ld_partners_host(codes, window, l, 0.0, None, mo)
        if rate == 0.0:                                                                       # nothing masked: both see the same genotypes
            assert np.array_equal(p_bed, p_panel) and np.array_equal(r_bed.view(np.uint64), r_panel.view(np.uint64))
            continue
        rows_p, counts_p = r_api.impute_ldknn_host(codes, p_panel, k, 1, 4)
        rows_b, counts_b = r_api.impute_ldknn_host(codes, p_bed, k, 1, 4)
        conc_p = float(np.mean(unpack(rows_p, n)[mask] == truth[mask]))
        conc_b = float(np.mean(unpack(rows_b, n)[mask] == truth[mask]))
        print("seed %d, %2.0f %% masked: partners from the panel %.4f, from the .bed file %.4f" % (seed, 100 * rate, conc_p, conc_b))
        assert counts_p.sum() == mask.sum() == counts_b.sum()
        assert not np.any(unpack(rows_b, n) == 1) and np.array_equal(unpack(rows_b, n)[~mask], codes[~mask])
