"""CPU: the host side of sample QC -- r_api.king_from_counts, king_degree, related_drop, sample_keep_mask, the inbreeding coefficient of
sample_stats_from_counts, the hwe= rule of marker_keep_mask -- on hand-made integers, and the argument errors of the four C entry
points, which are decided before a context is needed (ctx == NULL).  No device work."""
import ctypes as C

import numpy as np
import pytest

ERR_ARG = -3
I32P = C.POINTER(C.c_int32)


def counts_of(G):
    """ibs0, hethet of a small n x L matrix of -1 / 0 / +1 by the definition: pairs of opposite homozygotes, pairs of heterozygotes."""
    G = np.asarray(G)
    n = G.shape[0]
    ibs0, hethet = np.zeros((n, n), dtype=np.int32), np.zeros((n, n), dtype=np.int32)
    for i in range(n):
        for j in range(n):
            ibs0[i, j] = np.sum(G[i] * G[j] == -1)
            hethet[i, j] = np.sum((G[i] == 0) & (G[j] == 0))
    return ibs0, hethet


def test_king_from_counts_by_hand():
    from eagleeverything_amd import r_api
    G = np.array([[0, 0, 1, -1, 0, 1],
                  [0, 0, 1, -1, 0, 1],      # a duplicate of 0
                  [0, 1, -1, 1, 0, 0],
                  [1, 1, -1, -1, 1, 1],     # all homozygous
                  [-1, 1, 1, -1, -1, 1]])   # all homozygous
    ibs0, hethet = counts_of(G)
    phi = r_api.king_from_counts(ibs0, hethet)
    assert phi.dtype == np.float64 and phi.shape == (5, 5)
    assert phi[0, 1] == 0.5 and phi[1, 0] == 0.5 and phi[0, 0] == 0.5 and phi[2, 2] == 0.5
    # 0 and 2: hethet = 2 (markers 0, 4), ibs0 = 2 (markers 2, 3), h = 3 and 3
    assert phi[0, 2] == (2 - 2 * 2) / (3 + 3) and phi[2, 0] == phi[0, 2]
    # 0 and 3: hethet = 0, ibs0 = 1 (marker 2), h = 3 and 0
    assert phi[0, 3] == (0 - 2 * 1) / 3.0
    assert np.isnan(phi[3, 4]) and np.isnan(phi[4, 3]) and np.isnan(phi[3, 3]) and np.isnan(phi[4, 4])
    assert np.array_equal(np.isnan(phi), np.isnan(phi.T))


def test_degree_cuts():
    from eagleeverything_amd import r_api
    phi = [0.5, 0.3541, 0.354, 0.25, 0.1771, 0.177, 0.125, 0.08841, 0.0884, 0.0625, 0.04421, 0.0442, 0.0, -0.3, float("nan")]
    want = ["duplicate", "duplicate", "first", "first", "first", "second", "second", "second", "third", "third", "third", "unrelated",
            "unrelated", "unrelated", "unrelated"]
    assert r_api.king_degree(phi) == want


def test_related_drop_greedy():
    from eagleeverything_amd import r_api
    assert r_api.related_drop(np.zeros((0, 2), dtype=np.int64), 5).tolist() == []
    # a star around 2 and a separate pair: 2 (most pairs), then of (5, 6) the higher index; 1-based on return
    pairs = [[0, 2], [1, 2], [2, 3], [5, 6]]
    assert r_api.related_drop(pairs, 8).tolist() == [3, 7]
    # a path 0 - 1 - 2 - 3: 1 and 2 tie on two pairs -> 2 goes, then (0, 1) remains -> 1 goes
    assert r_api.related_drop([[0, 1], [1, 2], [2, 3]], 4).tolist() == [2, 3]
    # priority breaks ties (the lower goes) before the index does, but not the count
    prio = np.array([0.9, 0.99, 0.95, 0.5, 1.0, 0.7, 0.8, 1.0])
    assert r_api.related_drop(pairs, 8, priority=prio).tolist() == [3, 6]
    assert r_api.related_drop([[0, 1], [1, 2], [2, 3]], 4, priority=[1.0, 0.2, 0.3, 1.0]).tolist() == [2, 3]
    for bad in ([[0, 0]], [[0, 9]], [[-1, 2]]):
        with pytest.raises(ValueError):
            r_api.related_drop(bad, 4)
    # whatever is dropped, no pair survives
    rng = np.random.default_rng(3)
    pr = rng.integers(0, 30, size=(60, 2))
    pr = pr[pr[:, 0] != pr[:, 1]]
    gone = set((r_api.related_drop(pr, 30) - 1).tolist())
    assert all(i in gone or j in gone for i, j in pr.tolist())


def test_sample_keep_mask_and_drop_index():
    from eagleeverything_amd import r_api
    het = np.array([0.30, 0.31, 0.29, 0.30, 0.32, 0.28, 0.30, 0.60, 0.30, 0.05])
    n1 = np.round(het * 100).astype(np.int64)
    stats = r_api.sample_stats_from_counts(50 - n1 // 2, n1, 50 - (n1 - n1 // 2), n_missing=[0, 0, 0, 30, 0, 0, 0, 0, 1, 0])
    assert np.allclose(stats["het_rate"], het) and np.array_equal(stats["hom_count"], 100 - n1)
    assert np.allclose(stats["call_rate"], [1, 1, 1, 100 / 130, 1, 1, 1, 1, 100 / 101, 1])
    assert r_api.sample_keep_mask(stats).all()
    assert r_api.sample_keep_mask(stats, min_call_rate=0.95).tolist() == [True, True, True, False, True, True, True, True, True, True]
    mean, sd = het.mean(), het.std(ddof=1)
    want = np.abs(het - mean) <= 1.5 * sd
    assert want.sum() == 8 and not want[7] and not want[9]
    got = r_api.sample_keep_mask(stats, het_sd=1.5)
    assert np.array_equal(got, want)
    both = r_api.sample_keep_mask(stats, min_call_rate=0.95, het_sd=1.5)
    assert r_api.sample_drop_index(both).tolist() == [4, 8, 10]
    with pytest.raises(ValueError):
        r_api.sample_keep_mask({"n0": stats["n0"], "het_rate": het}, min_call_rate=0.9)


def test_inbreeding_coefficient_formula():
    """F_i = (O_i - E) / (L - E), E = sum_j 1 - 2 p_j (1 - p_j) 2n / (2n - 1), on a 4 x 3 panel worked by hand."""
    from eagleeverything_amd import r_api
    G = np.array([[-1, 0, 1], [1, 0, 1], [0, 0, 1], [-1, 1, -1]])   # individuals x markers
    n, L = G.shape
    mstats = r_api.marker_stats_from_counts(*[np.sum(G == v, axis=0) for v in (-1, 0, 1)])
    p = np.array([3 / 8, 5 / 8, 6 / 8])                             # (2 n2 + n1) / 2n per marker
    assert np.allclose(mstats["freq"], p)
    E = sum(1 - 2 * pj * (1 - pj) * (2 * n) / (2 * n - 1) for pj in p)
    s = r_api.sample_stats_from_counts(*[np.sum(G == v, axis=1) for v in (-1, 0, 1)], marker_stats=mstats)
    O = np.array([2, 2, 1, 3])
    assert np.array_equal(s["hom_count"], O)
    np.testing.assert_allclose(s["F"], (O - E) / (L - E), rtol=1e-14)
    assert abs(s["expected_hom"] - E) < 1e-14
    assert "F" not in r_api.sample_stats_from_counts([1], [1], [1])


def test_marker_keep_mask_hwe_rule():
    from eagleeverything_amd import r_api
    stats = r_api.marker_stats_from_counts([10, 50, 0, 30], [20, 0, 0, 40], [10, 50, 40, 30])
    with pytest.raises(ValueError):
        r_api.marker_keep_mask(stats, hwe=1e-3)
    stats["hwe_p"] = np.array([1.0, 1e-30, 1.0, 1e-3])
    assert r_api.marker_keep_mask(stats).all()                                            # the default is unchanged
    assert r_api.marker_keep_mask(stats, hwe=1e-3).tolist() == [True, False, True, True]  # p < hwe drops, p == hwe stays
    assert r_api.marker_keep_mask(stats, hwe=1e-3, drop_monomorphic=True).tolist() == [True, False, False, True]


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()
    dims = (C.c_long * 2)(5, 7)
    zero = (C.c_long * 2)(0, 7)
    neg = (C.c_long * 2)(5, -1)
    huge = (C.c_long * 2)(5, 1 << 31)
    out = (C.c_int32 * 200)()
    out2 = (C.c_int32 * 200)()
    p = (C.c_double * 8)()
    path = str(tmp_path / "M.ascii").encode()

    def text():
        return L.eagle_open_error().decode()
    for fn, name in ((L.eagle_sample_counts, "sample_counts"), (L.eagle_bed_sample_counts, "bed_sample_counts")):
        assert fn(None, None, dims, 8.0, out) == ERR_ARG and name in text() and "NULL" in text()
        assert fn(None, path, None, 8.0, out) == ERR_ARG
        assert fn(None, path, dims, 8.0, None) == ERR_ARG
        assert fn(None, path, zero, 8.0, out) == ERR_ARG and "dims" in text()
        assert fn(None, path, neg, 8.0, out) == ERR_ARG
        assert fn(None, path, dims, 8.0, out) == ERR_ARG and "no context" in text()
    fn = L.eagle_sample_ibs
    assert fn(None, None, dims, 8.0, out, out2) == ERR_ARG and "sample_ibs" in text()
    assert fn(None, path, dims, 8.0, None, out2) == ERR_ARG
    assert fn(None, path, dims, 8.0, out, None) == ERR_ARG
    assert fn(None, path, zero, 8.0, out, out2) == ERR_ARG and "dims" in text()
    assert fn(None, path, huge, 8.0, out, out2) == ERR_ARG
    assert fn(None, path, dims, 8.0, out, out2) == ERR_ARG and "no context" in text()
    cnt = (C.c_int32 * 8)(10, 20, 10, 0, 5, 5, 5, 0)
    fn = L.eagle_hwe_exact
    assert fn(None, None, 2, 4, p) == ERR_ARG and "hwe_exact" in text()
    assert fn(None, cnt, 2, 4, None) == ERR_ARG
    assert fn(None, cnt, 0, 4, p) == ERR_ARG
    assert fn(None, cnt, 2, 2, p) == ERR_ARG and "stride" in text()
    assert fn(None, cnt, 2, 5, p) == ERR_ARG
    bad = (C.c_int32 * 6)(10, -1, 10, 1, 1, 1)
    assert fn(None, bad, 2, 3, p) == ERR_ARG and "negative" in text()
    big = (C.c_int32 * 3)(1 << 30, 1, 0)
    assert fn(None, big, 1, 3, p) == ERR_ARG
    assert fn(None, cnt, 2, 4, p) == ERR_ARG and "no context" in text()
    assert fn(None, cnt, 2, 3, p) == ERR_ARG and "no context" in text()
