"""CPU: the numpy restatements of LD-kNNi (r_api.ld_partners_host, r_api.impute_ldknn_host; include/eagle_hip.h section 1b'''iii)
against plain loops of the definitions, the popcount identity the kernel computes d and ov with, and what the method is for: on a
founder-mosaic panel it fills masked genotypes far better than genome-wide neighbours do.  No device work."""
import functools

import numpy as np
import pytest

DOSAGE = {0: 0, 2: 1, 3: 2}
CODE = {0: 0, 1: 2, 2: 3}
GVAL = {0: -1, 1: 0, 2: 0, 3: 1}


# ---- plain loops of the definitions ----
def loop_partners(Mt8, window, l, min_r2, chrom):
    L, n = Mt8.shape
    G = [[int(x) for x in row] for row in Mt8]
    s = [sum(r) for r in G]
    v = [n * sum(x * x for x in r) - sr * sr for r, sr in zip(G, s)]
    part = np.full((L, l), -1, dtype=np.int32)
    r2o = np.zeros((L, l))
    for i in range(L):
        cand = []
        for j in range(L):
            if j == i or abs(j - i) > window or v[i] <= 0 or v[j] <= 0:
                continue
            if chrom is not None and chrom[i] != chrom[j]:
                continue
            c = n * sum(a * b for a, b in zip(G[i], G[j])) - s[i] * s[j]
            r2 = (np.float64(c) * np.float64(c)) / (np.float64(v[i]) * np.float64(v[j]))
            if r2 >= min_r2:
                cand.append((-r2, abs(j - i), j))
        cand.sort()
        for t, (nr2, _, j) in enumerate(cand[:l]):
            part[i, t], r2o[i, t] = j, -nr2
    return part, r2o


def loop_impute(codes, partners, k, min_votes, min_overlap):
    L, n = codes.shape
    out = codes.copy()
    counts = np.zeros((L, 2), dtype=np.int32)
    for m in range(L):
        called = [j for j in range(n) if codes[m, j] != 1]
        if called:
            c, s = len(called), sum(DOSAGE[int(codes[m, j])] for j in called)
            fb = CODE[(2 * s + c) // (2 * c)]
        else:
            fb = 2
        P = [int(p) for p in partners[m] if p >= 0]
        for i in range(n):
            if codes[m, i] != 1:
                continue
            keys = []
            for j in called:
                ov = d = 0
                for p in P:
                    a, b = int(codes[p, i]), int(codes[p, j])
                    if a != 1 and b != 1:
                        ov += 1
                        d += (GVAL[a] - GVAL[b]) ** 2
                if ov >= min_overlap:
                    keys.append(((d * 4096) // ov << 32) | j)
            keys.sort()
            voters = [key & 0xffffffff for key in keys[:k]]
            c, s = len(voters), sum(DOSAGE[int(codes[m, j])] for j in voters)
            if c >= min_votes:
                out[m, i] = CODE[(2 * s + c) // (2 * c)]
                counts[m, 0] += 1
            else:
                out[m, i] = fb
                counts[m, 1] += 1
    return out, counts


# ---- ld_partners_host ----
@functools.lru_cache(maxsize=None)
def partner_panel():
    rng = np.random.default_rng(5)
    n, L = 40, 120
    Mt8 = rng.integers(-1, 2, size=(L, n)).astype(np.int8)
    Mt8[7], Mt8[61] = 1, 0                   # two monomorphic markers
    Mt8[26] = Mt8[30] = Mt8[28]              # identical markers: seen from 28 the two others tie (r2 = 1, |j - i| = 2): the smaller j first;
                                             # seen from 26 they tie in r2 alone: the smaller |j - i| first
    Mt8[59] = Mt8[56]                        # identical across the chrom split below
    Mt8.setflags(write=False)
    return Mt8


@pytest.mark.parametrize("window,l,min_r2,split", [(50, 16, 0.0, False), (5, 32, 0.0, True), (256, 7, 0.02, True), (1, 1, 0.0, False), (3, 4, 0.5, False)])
def test_ld_partners_host_equals_the_double_loop(window, l, min_r2, split):
    from eagleeverything_amd import r_api
    Mt8 = partner_panel()
    L = Mt8.shape[0]
    chrom = np.where(np.arange(L) < 58, 3, 1) if split else None
    part, r2 = r_api.ld_partners_host(Mt8, window, l, min_r2, chrom)
    want, want_r2 = loop_partners(Mt8, window, l, min_r2, chrom)
    assert part.dtype == np.int32 and part.shape == (L, l) and r2.dtype == np.float64
    assert np.array_equal(part, want) and np.array_equal(r2, want_r2)               # r2: the same bits
    assert (part[[7, 61]] == -1).all() and not np.any(part == 7) and not np.any(part == 61)
    if window >= 2 and l >= 2:
        assert part[28, :2].tolist() == [26, 30] and r2[28, :2].tolist() == [1.0, 1.0]
        assert part[26, 0] == 28 and part[30, 0] == 28
    if window >= 4 and l >= 2:
        assert part[26, :2].tolist() == [28, 30] and part[30, :2].tolist() == [28, 26] and r2[26, :2].tolist() == [1.0, 1.0]
    if split:
        assert not np.any((part[:58] >= 58)) and not np.any((part[58:] >= 0) & (part[58:] < 58))
    if window < l // 2:
        assert (part[:, 2 * window:] == -1).all() and (r2[part == -1] == 0.0).all()  # fewer candidates than l


def test_ld_partners_host_refuses_bad_arguments():
    from eagleeverything_amd import r_api
    Mt8 = partner_panel()
    for kw in (dict(window=0), dict(window=257), dict(l=0), dict(l=33), dict(min_r2=-0.1), dict(min_r2=1.5), dict(chrom=np.zeros(3))):
        a = dict(window=5, l=4, min_r2=0.0, chrom=None)
        a.update(kw)
        with pytest.raises(ValueError):
            r_api.ld_partners_host(Mt8, a["window"], a["l"], a["min_r2"], a["chrom"])
    one = r_api.ld_partners_host(Mt8[:1], 50, 16, 0.0)
    assert (one[0] == -1).all() and one[0].shape == (1, 16)


# ---- impute_ldknn_host ----
@functools.lru_cache(maxsize=None)
def impute_panel():
    rng = np.random.default_rng(11)
    n, L, l = 23, 60, 6
    codes = np.array([0, 2, 3], dtype=np.uint8)[rng.integers(0, 3, size=(L, n))]
    codes[rng.random((L, n)) < 0.2] = 1
    codes[9, :] = 1                                                  # a marker without any call
    partners = np.full((L, l), -1, dtype=np.int32)
    for m in range(L):
        near = [j for j in range(max(0, m - 5), min(L, m + 6)) if j != m]
        pick = rng.permutation(near)[:rng.integers(1, l + 1)]
        partners[m, :pick.size] = pick
    partners[17, :] = -1                                             # no partners: every missing genotype of marker 17 by fallback
    partners[20, :3] = (22, 22, 19)                                  # a repeated partner counts twice
    codes.setflags(write=False)
    partners.setflags(write=False)
    return codes, partners


@pytest.mark.parametrize("k,min_votes,min_overlap", [(1, 1, 1), (5, 1, 1), (5, 2, 4), (64, 1, 2), (3, 4, 1), (5, 1, 6)])
def test_impute_ldknn_host_equals_the_triple_loop(k, min_votes, min_overlap):
    from eagleeverything_amd import r_api
    codes, partners = impute_panel()
    L, n = codes.shape
    rows, counts = r_api.impute_ldknn_host(codes, partners, k, min_votes, min_overlap)
    want, want_counts = loop_impute(codes, partners, k, min_votes, min_overlap)
    assert np.array_equal(rows, r_api.pack_bed_codes(want)) and np.array_equal(counts, want_counts)
    assert counts.dtype == np.int32 and np.array_equal(counts.sum(axis=1), (codes == 1).sum(axis=1))
    assert counts[17].tolist() == [0, int((codes[17] == 1).sum())] and counts[17, 1] > 0        # an all -1 partner row
    assert counts[9].tolist() == [0, n] and (want[9] == 2).all()                               # no call: heterozygous
    if min_votes > k:
        assert not counts[:, 0].any()
    if min_overlap == 4:                                             # above what some pairs have, below what others have
        assert counts[:, 0].any() and counts[np.arange(L) != 9][:, 1].sum() > counts[17, 1]
    assert not np.any(want == 1) and np.array_equal(want[codes != 1], codes[codes != 1])


def test_impute_ldknn_host_refuses_bad_arguments():
    from eagleeverything_amd import r_api
    codes, partners = impute_panel()
    out = np.array(partners)
    out[3, 1] = 60
    for p, k, mv, mo in ((partners, 0, 1, 1), (partners, 65, 1, 1), (partners, 5, 0, 1), (partners, 5, 1, 0), (partners, 5, 1, 33),
                         (out, 5, 1, 1), (partners[:10], 5, 1, 1), (np.zeros((60, 33), dtype=np.int32), 5, 1, 1)):
        with pytest.raises(ValueError):
            r_api.impute_ldknn_host(codes, p, k, mv, mo)
    wide, far = np.zeros((300, 4), dtype=np.uint8), np.full((300, 2), -1, dtype=np.int32)
    far[10, 1] = 266
    r_api.impute_ldknn_host(wide, far, 5, 1, 1)                      # 256 rows away: the limit
    far[10, 1] = 267
    with pytest.raises(ValueError):
        r_api.impute_ldknn_host(wide, far, 5, 1, 1)


def test_popcount_identity_over_all_code_pairs():
    """called / hom / homA2 words, bit p = partner p:  ov = popc(B),  d = popc(B & (hom_i ^ hom_j)) + 4 popc(hom_i & hom_j & (homA2_i ^
    homA2_j)),  B = called_i & called_j -- against the direct sums, with every one of the 4^4 (code_i, code_j) pairs at two partners."""
    def words(cs):
        return (sum((c != 1) << p for p, c in enumerate(cs)), sum((c in (0, 3)) << p for p, c in enumerate(cs)),
                sum((c == 3) << p for p, c in enumerate(cs)))

    def popc(x):
        return bin(x).count("1")
    seen = 0
    for a0 in range(4):
        for a1 in range(4):
            for b0 in range(4):
                for b1 in range(4):
                    ci, hi, ai = words((a0, a1))
                    cj, hj, aj = words((b0, b1))
                    B = ci & cj
                    ov = popc(B)
                    d = popc(B & (hi ^ hj)) + 4 * popc(hi & hj & (ai ^ aj))
                    pairs = [(a, b) for a, b in ((a0, b0), (a1, b1)) if a != 1 and b != 1]
                    assert ov == len(pairs) and d == sum((GVAL[a] - GVAL[b]) ** 2 for a, b in pairs)
                    seen += 1
    assert seen == 256


# ---- what it is for ----
def mosaic_panel(seed, n=96, L=400, founders=8, seg=40, rate=0.05):
    """codes uint8 (L, n) with `rate` masked, and the truth: two haplotypes per individual, each a mosaic of inbred founders whose
    segment lengths are geometric with mean `seg` markers."""
    rng = np.random.default_rng(seed)
    F = rng.integers(0, 2, size=(founders, L))

    def hap():
        h = np.empty(L, dtype=np.int64)
        pos = 0
        while pos < L:
            ln = int(rng.geometric(1.0 / seg))
            h[pos:pos + ln] = F[rng.integers(founders), pos:pos + ln]
            pos += ln
        return h
    dose = np.stack([hap() + hap() for _ in range(n)], axis=1)                     # (L, n) in {0, 1, 2}
    truth = np.array([0, 2, 3], dtype=np.uint8)[dose]
    codes = truth.copy()
    mask = rng.random((L, n)) < rate
    codes[mask] = 1
    return codes, truth, mask


def unpack(rows, n):
    return np.stack([(rows >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(rows.shape[0], -1)[:, :n]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_local_neighbours_beat_genome_wide_ones_on_a_founder_mosaic(seed):
    from eagleeverything_amd import r_api
    codes, truth, mask = mosaic_panel(seed)
    L, n = codes.shape
    k = 5
    Mt8 = np.array([-1, 0, 0, 1], dtype=np.int8)[codes]                            # the ingested panel: missing = heterozygous
    G = Mt8.astype(np.int64)
    d = ((G[:, :, None] - G[:, None, :]) ** 2).sum(axis=0).astype(np.int32)        # knn_distance's d: sum (g_i - g_j)^2
    rows_g, _ = r_api.impute_knn_host(codes, r_api.knn_rows_host(d, 64), k, 1)
    partners, _ = r_api.ld_partners_host(Mt8, 50, 16, 0.0)
    rows_l, counts = r_api.impute_ldknn_host(codes, partners, k, 1, 4)
    conc_g = float(np.mean(unpack(rows_g, n)[mask] == truth[mask]))
    conc_l = float(np.mean(unpack(rows_l, n)[mask] == truth[mask]))
    print("seed %d: genome-wide kNN %.3f, LD-kNNi %.3f" % (seed, conc_g, conc_l))
    assert counts.sum() == mask.sum()
    assert conc_l >= conc_g + 0.10, (conc_g, conc_l)
