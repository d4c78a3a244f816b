"""CPU: the numpy restatements of kNN imputation (r_api.knn_distance, knn_rows_host, impute_knn_host) against plain Python loops
of the definitions in include/eagle_hip.h section 1b'''i, and the condition on the method itself: on a panel of close relatives the
kNN fill recovers masked genotypes better than the heterozygote fill and than the per-marker fallback.  Every comparison of the
restatements is exact (integers and bytes).  No device work."""
import numpy as np
import pytest

DOSE = {0: 0, 2: 1, 3: 2}
CODE = {0: 0, 1: 2, 2: 3}


def loop_impute(codes, nbr, k, min_votes):
    """The definition, one genotype at a time -> (bytes of the marker rows, [[by vote, by fallback] per marker])."""
    L, n = len(codes), len(codes[0])
    rb = (n + 3) // 4
    out, counts = bytearray(L * rb), []
    for m in range(L):
        row = [int(v) for v in codes[m]]
        called = [c for c in row if c != 1]
        c_m, s_m = len(called), sum(DOSE[c] for c in called)
        fallback = CODE[(2 * s_m + c_m) // (2 * c_m)] if c_m else 2
        votes = fallbacks = 0
        for i in range(n):
            g = row[i]
            if g == 1:
                c = s = 0
                for j in nbr[i]:
                    j = int(j)
                    if j < 0 or row[j] == 1:
                        continue
                    c += 1
                    s += DOSE[row[j]]
                    if c == k:
                        break
                if c >= min_votes:
                    g = CODE[(2 * s + c) // (2 * c)]
                    votes += 1
                else:
                    g = fallback
                    fallbacks += 1
            out[m * rb + i // 4] |= g << (2 * (i % 4))
        counts.append([votes, fallbacks])
    return bytes(out), counts


def random_codes(rng, L, n, rate):
    codes = np.array([0, 2, 3], dtype=np.uint8)[rng.integers(0, 3, size=(L, n))]
    codes[rng.random((L, n)) < rate] = 1
    return codes


def random_nbr(rng, n, K):
    """A neighbour table of the shape knn_rows makes: min(K, n - 1) distinct others in random order, then -1."""
    nbr = np.full((n, K), -1, dtype=np.int32)
    keff = min(K, n - 1)
    for i in range(n):
        others = np.array([j for j in range(n) if j != i], dtype=np.int32)
        nbr[i, :keff] = rng.permutation(others)[:keff]
    return nbr


@pytest.mark.parametrize("n", [1, 2, 5, 64, 67])
@pytest.mark.parametrize("rate", [0.0, 0.1, 1.0])
def test_impute_knn_host_equals_the_loop(n, rate):
    from eagleeverything_amd import r_api
    L = 9
    rng = np.random.default_rng(1000 * n + int(10 * rate))
    codes = random_codes(rng, L, n, rate)
    if rate == 0.1 and n >= 5:
        codes[3, :] = 1                      # a marker without a call
        codes[4, : n // 2] = 1               # a marker where whole neighbour lists are missing
    for K, k, min_votes in ((1, 1, 1), (3, 2, 1), (3, 3, 3), (70, 5, 2), (70, 70, 1)):
        nbr = random_nbr(rng, n, K)
        rows, counts = r_api.impute_knn_host(codes, nbr, k, min_votes)
        want_bytes, want_counts = loop_impute(codes.tolist(), nbr.tolist(), k, min_votes)
        assert rows.dtype == np.uint8 and rows.shape == (L, (n + 3) // 4)
        assert rows.tobytes() == want_bytes
        assert counts.dtype == np.int32 and counts.tolist() == want_counts
        assert np.array_equal(counts.sum(axis=1), (codes == 1).sum(axis=1))
        assert not np.any(np.stack([(rows >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(L, -1)[:, :n] == 1)


def test_impute_knn_host_by_hand():
    from eagleeverything_amd import r_api
    #                 i = 0  1  2  3  4
    codes = np.array([[1, 0, 3, 3, 2],      # i = 0 missing: neighbours 1, 2, 3 -> dosages 0, 2, 2: (2 * 4 + 3) // 6 = 1 -> het
                      [1, 1, 3, 1, 0],      # i = 0: neighbours 1, 3 missing, 2 votes alone -> 3; with min_votes = 2 the marker's mean
                      [1, 1, 1, 1, 1],      # no call at all: het
                      [0, 2, 3, 3, 0]],     # nothing missing
                     dtype=np.uint8)
    nbr = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2]], dtype=np.int32)
    rows, counts = r_api.impute_knn_host(codes, nbr, 3, 1)
    dec = np.stack([(rows >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(4, -1)
    assert dec[0].tolist() == [2, 0, 3, 3, 2, 0, 0, 0]
    # marker 1: i = 0 <- {2}: 3;  i = 1 <- {0: missing, 2: 3, 3: missing}: 3;  i = 3 <- {2}: 3
    assert dec[1].tolist() == [3, 3, 3, 3, 0, 0, 0, 0]
    assert dec[2].tolist() == [2, 2, 2, 2, 2, 0, 0, 0]
    assert dec[3].tolist() == [0, 2, 3, 3, 0, 0, 0, 0]
    assert counts.tolist() == [[1, 0], [3, 0], [0, 5], [0, 0]]
    rows2, counts2 = r_api.impute_knn_host(codes, nbr, 3, 2)
    dec2 = np.stack([(rows2 >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(4, -1)
    # marker 1 by its own calls: c = 2, s = 2 + 0 -> (4 + 2) // 4 = 1 -> het
    assert dec2[1].tolist() == [2, 2, 3, 2, 0, 0, 0, 0] and counts2.tolist() == [[1, 0], [0, 3], [0, 5], [0, 0]]
    for bad in ((nbr, 0, 1), (nbr, 4, 1), (nbr, 1, 0), (nbr[:4], 1, 1), (nbr + 3, 1, 1)):
        with pytest.raises(ValueError):
            r_api.impute_knn_host(codes, *bad)


def test_bed_codes_round_trip(tmp_path):
    from eagleeverything_amd import r_api, synth
    rng = np.random.default_rng(5)
    for n in (1, 4, 7):
        Mt8 = rng.integers(-1, 2, size=(6, n)).astype(np.int8)
        miss = rng.random((6, n)) < 0.3
        bed = synth.write_bed(str(tmp_path / ("p%d" % n)), Mt8, missing=miss)
        codes = r_api.read_bed_codes(bed, (n, 6))
        want = np.array([0, 2, 3], dtype=np.uint8)[Mt8 + 1]
        want[miss] = 1
        assert np.array_equal(codes, want)
        assert b"\x6c\x1b\x01" + r_api.pack_bed_codes(codes).tobytes() == open(bed, "rb").read()
        with pytest.raises(ValueError):
            r_api.read_bed_codes(bed, (n, 5))


def test_knn_rows_host_equals_sorted_with_ties():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 9, 40):
        d = rng.integers(0, 6, size=(n, n)).astype(np.int32)       # few values: ties in every row
        d = np.minimum(d, d.T)
        if n >= 9:
            d[0, :] = 7                                             # a row of equal distances: index order
            d[1, 2:6] = 0
        for K in (1, 4, n - 1 if n > 1 else 1, n + 3):
            got = r_api.knn_rows_host(d, K)
            assert got.dtype == np.int32 and got.shape == (n, K)
            for i in range(n):
                order = [j for _, j in sorted((int(d[i, j]), j) for j in range(n) if j != i)][:K]
                assert got[i].tolist() == order + [-1] * (K - len(order))
    with pytest.raises(ValueError):
        r_api.knn_rows_host(np.zeros((3, 3), dtype=np.int32), 0)
    with pytest.raises(ValueError):
        r_api.knn_rows_host(np.zeros((3, 3), dtype=np.int32), 257)


def test_knn_distance_is_the_squared_difference():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(3)
    G = rng.integers(-1, 2, size=(13, 57)).astype(np.int64)
    G[4] = G[2]                                                     # a duplicate: distance 0
    ibs0 = np.array([[np.sum(G[i] * G[j] == -1) for j in range(13)] for i in range(13)], dtype=np.int32)
    hethet = np.array([[np.sum((G[i] == 0) & (G[j] == 0)) for j in range(13)] for i in range(13)], dtype=np.int32)
    d = r_api.knn_distance(ibs0, hethet)
    assert d.dtype == np.int32
    assert np.array_equal(d, ((G[:, None, :] - G[None, :, :]) ** 2).sum(axis=2))
    assert d[2, 4] == 0 and not np.any(np.diagonal(d))


# ---- the condition on the method: 8 founders x 12 copies, 2 % of every copy redrawn, 5 % masked ----
def relatives_panel(seed):
    rng = np.random.default_rng(seed)
    founders = rng.integers(-1, 2, size=(8, 400))
    G = np.repeat(founders, 12, axis=0)
    redraw = rng.random(G.shape) < 0.02
    G = np.where(redraw, rng.integers(-1, 2, size=G.shape), G).astype(np.int8)
    mask = rng.random(G.shape) < 0.05
    return G, mask


def test_knn_beats_het_fill_and_marker_mean():
    """Measured at this seed (written into DESIGN 4.8e): kNN 0.9850, per-marker fallback 0.3500, heterozygote fill 0.3335; four
    other seeds gave kNN 0.984 .. 0.990 against at most 0.364 for the other two, so the strict inequalities have a wide margin."""
    from eagleeverything_amd import r_api
    G, mask = relatives_panel(0)
    n, L = G.shape
    assert (n, L) == (96, 400)
    ingested = np.where(mask, 0, G).astype(np.int64)               # what ingestion makes of the file: missing -> het
    ibs0 = (ingested[:, None, :] * ingested[None, :, :] == -1).sum(axis=2).astype(np.int32)
    hethet = ((ingested[:, None, :] == 0) & (ingested[None, :, :] == 0)).sum(axis=2).astype(np.int32)
    nbr = r_api.knn_rows_host(r_api.knn_distance(ibs0, hethet), 32)
    codes = np.array([0, 2, 3], dtype=np.uint8)[G.T + 1]
    codes[mask.T] = 1
    value = np.array([-1, 99, 0, 1])

    def concordance(rows):
        dec = np.stack([(rows >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(L, -1)[:, :n]
        assert not np.any(dec == 1)
        filled = value[dec].T
        assert np.array_equal(filled[~mask], G[~mask])             # called genotypes are copied
        return float(np.mean(filled[mask] == G[mask]))

    rows, counts = r_api.impute_knn_host(codes, nbr, 5, 1)
    knn = concordance(rows)
    rows_fb, counts_fb = r_api.impute_knn_host(codes, np.full((n, 1), -1, dtype=np.int32), 1, 1)   # no neighbours: the fallback alone
    assert counts_fb[:, 0].sum() == 0 and counts_fb[:, 1].sum() == mask.sum() == counts.sum()
    marker_mean = concordance(rows_fb)
    het = float(np.mean(G[mask] == 0))
    print("concordance with the masked truth: kNN %.4f, per-marker fallback %.4f, heterozygote fill %.4f" % (knn, marker_mean, het))
    assert knn > het and knn > marker_mean
