"""CPU: the numpy restatement of the pairwise-complete counts (r_api.bed_ibs_host, king_from_pair_counts) against a plain double loop
over pairs and markers of the definitions in include/eagle_hip.h section 1b'''ii, and what the counts are for: a duplicated individual
whose two copies miss different genotypes is a duplicate (phi = 0.5 exactly) by the pairwise-complete counts and a first-degree relative
by the het-filled panel's.  Every comparison is exact.  No device work."""
import numpy as np
import pytest

G_OF_CODE = {0: -1, 2: 0, 3: 1}
NO_OVERLAP = 0xFFFFFFFE


def loop_counts(codes, include=None, min_overlap=1):
    """The definition, one pair and one marker at a time -> five lists of lists."""
    L, n = len(codes), len(codes[0])
    used = [m for m in range(L) if include is None or include[m]]
    out = [[[0] * n for _ in range(n)] for _ in range(5)]
    for i in range(n):
        for j in range(n):
            both = ibs0 = hethet = hetsum = sq = 0
            for m in used:
                a, b = int(codes[m][i]), int(codes[m][j])
                if a == 1 or b == 1:
                    continue
                both += 1
                ga, gb = G_OF_CODE[a], G_OF_CODE[b]
                ibs0 += ga * gb == -1
                hethet += a == 2 and b == 2
                hetsum += (a == 2) + (b == 2)
                sq += (ga - gb) ** 2
            out[0][i][j], out[1][i][j], out[2][i][j], out[3][i][j] = both, ibs0, hethet, hetsum
            assert sq == 4 * ibs0 + hetsum - 2 * hethet
            out[4][i][j] = sq * len(used) // both if both >= min_overlap else NO_OVERLAP
    return out


def random_codes(rng, L, n, rate):
    codes = np.array([0, 2, 3], dtype=np.uint8)[rng.integers(0, 3, size=(L, n))]
    codes[rng.random((L, n)) < rate] = 1
    return codes


@pytest.mark.parametrize("min_overlap", [1, 40])
def test_bed_ibs_host_equals_the_loop(min_overlap):
    from eagleeverything_amd import r_api
    n, L = 7, 60
    rng = np.random.default_rng(60)
    codes = random_codes(rng, L, n, 0.2)
    codes[:, 5] = 1                                   # an individual without a call
    codes[7, :] = 1                                   # a marker without a call
    codes[8, :5] = np.array([0, 3, 2, 2, 0])          # a marker without a missing code (but individual 5's)
    for include in (None, rng.random(L) < 0.5, np.zeros(L, dtype=bool)):
        got = r_api.bed_ibs_host(codes, include=include, min_overlap=min_overlap)
        want = loop_counts(codes.tolist(), None if include is None else include.tolist(), min_overlap)
        for k in range(4):
            assert got[k].dtype == np.int32 and got[k].shape == (n, n) and got[k].tolist() == want[k]
        assert got[4].dtype == np.uint32 and got[4].tolist() == want[4]
        if include is not None:                       # indices name the same markers as the mask
            idx = r_api.bed_ibs_host(codes, include=np.flatnonzero(include), min_overlap=min_overlap)
            assert all(np.array_equal(a, b) for a, b in zip(idx, got))
    ncalled, ibs0, hethet, hetsum, dist = r_api.bed_ibs_host(codes)
    assert np.array_equal(np.diagonal(ncalled), (codes != 1).sum(axis=0)) and not np.any(np.diagonal(ibs0))
    assert np.array_equal(np.diagonal(hethet), (codes == 2).sum(axis=0)) and np.array_equal(np.diagonal(hetsum), 2 * np.diagonal(hethet))
    with pytest.raises(ValueError):
        r_api.bed_ibs_host(codes, min_overlap=0)
    with pytest.raises(ValueError):
        r_api.bed_ibs_host(codes, include=np.ones(L + 1, dtype=bool))
    with pytest.raises(ValueError):
        r_api.bed_ibs_host(codes, include=[0, L])


def test_duplicate_with_independent_masks_is_a_duplicate():
    """n = 7, L = 300, individuals 1 and 4 are one genotype vector with 20 % of each copy masked independently."""
    from eagleeverything_amd import r_api
    n, L = 7, 300
    rng = np.random.default_rng(20)
    G = rng.integers(-1, 2, size=(n, L))
    G[4] = G[1]
    mask = np.zeros((n, L), dtype=bool)
    mask[1], mask[4] = rng.random(L) < 0.2, rng.random(L) < 0.2
    codes = np.array([0, 2, 3], dtype=np.uint8)[G.T + 1]
    codes[mask.T] = 1
    ncalled, ibs0, hethet, hetsum, dist = r_api.bed_ibs_host(codes)
    phi = r_api.king_from_pair_counts(ibs0, hethet, hetsum)
    assert phi.dtype == np.float64 and phi[1, 4] == 0.5 and phi[4, 1] == 0.5 and np.all(np.diagonal(phi) == 0.5)
    assert dist[1, 4] == 0 and ncalled[1, 4] == np.sum(~mask[1] & ~mask[4]) < L
    filled = np.where(mask, 0, G)                     # the ingested panel: missing -> heterozygous
    a = (filled[:, None, :] * filled[None, :, :] == -1).sum(axis=2)
    h = ((filled[:, None, :] == 0) & (filled[None, :, :] == 0)).sum(axis=2)
    old = r_api.king_from_counts(a, h)
    print("duplicate pair: pairwise-complete phi %.4f, het-filled phi %.4f" % (phi[1, 4], old[1, 4]))
    assert old[1, 4] < 0.45
    others = [(i, j) for i in range(n) for j in range(n) if i != j and {i, j} != {1, 4}]
    assert all(phi[i, j] < 0.354 for i, j in others)  # nobody else is a duplicate


def test_individual_without_a_call_comes_last():
    from eagleeverything_amd import r_api
    n, L = 9, 80
    rng = np.random.default_rng(9)
    codes = random_codes(rng, L, n, 0.1)
    codes[:, 3] = 1
    ncalled, ibs0, hethet, hetsum, dist = r_api.bed_ibs_host(codes)
    assert not np.any(ncalled[3]) and not np.any(ncalled[:, 3])
    phi = r_api.king_from_pair_counts(ibs0, hethet, hetsum)
    assert np.all(np.isnan(phi[3])) and np.all(np.isnan(phi[:, 3]))
    assert np.all(dist[3] == NO_OVERLAP) and np.all(dist[:, 3] == NO_OVERLAP)
    for K in (1, 3, n - 1, n + 2):
        nbr = r_api.knn_rows_host(dist, K)            # the uint32 matrix as it is
        keff = min(K, n - 1)
        for i in range(n):
            if i == 3:
                assert nbr[3, :keff].tolist() == [j for j in range(n) if j != 3][:keff]     # all equal: index order
            elif keff == n - 1:
                assert nbr[i, keff - 1] == 3
            else:
                assert 3 not in nbr[i].tolist()
            order = [j for _, j in sorted((int(dist[i, j]), j) for j in range(n) if j != i)][:K]
            assert nbr[i].tolist() == order + [-1] * (K - len(order))


def test_relatedness_refuses_a_marker_count_mismatch(tmp_path):
    from eagleeverything_amd import r_api, synth
    n, L = 6, 10
    rng = np.random.default_rng(1)
    Mt8 = rng.integers(-1, 2, size=(L, n)).astype(np.int8)
    bed = synth.write_bed(str(tmp_path / "p"), Mt8, missing=rng.random((L, n)) < 0.2)
    geno = {"asciifileM": str(tmp_path / "M.ascii"), "asciifileMt": str(tmp_path / "Mt.ascii"), "dim_of_ascii_M": [n, L - 3]}
    with pytest.raises(ValueError, match="include"):
        r_api.Relatedness(geno, bed=bed)
    with pytest.raises(ValueError, match="include"):
        r_api.Relatedness(geno, bed=str(tmp_path / "p"), include=np.arange(L - 2))       # names 8 markers, the panel holds 7
    with pytest.raises(ValueError):
        r_api.Relatedness(geno, bed=bed, include=[0, L])
