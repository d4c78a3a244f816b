"""CPU: r_api.ibd_host -- the vectorised numpy restatement of the pairwise IBD-type segments (include/eagle_hip.h section 1b'''vii) that
the GPU tests compare the device with -- against plain loops of the definitions (ibd_truth.ibd_loops), on random small cases and on hand
cases at every threshold of the rule; then ibd_incidence, `shared` and ibd_kinship.  Everything is integers: every comparison is ==."""
import numpy as np
import pytest

import ibd_truth as T


def same(got, want, what):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[1].ndim == 2 and got[1].shape[1] == 6, what
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), (what, "pair", got[0], want[0])
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), (what, "seg", got[1][:8], want[1][:8])


def test_ibd_host_equals_the_loops_on_random_small_cases():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(2027)
    some = merged = 0
    for case in range(300):
        n, L = int(rng.integers(2, 6)), int(rng.integers(1, 61))
        het = float(rng.choice([0.0, 0.1, 0.5]))
        g = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(L, n), p=[(1 - het) * 0.7, het, (1 - het) * 0.3])
        called = None
        if case % 3 == 0:
            called = rng.random((L, n)) >= 0.15
            g = np.where(called, g, 0).astype(np.int8)
        chrom = pos = None
        if case % 2:
            chrom = np.sort(rng.integers(0, 3, L)).astype(np.int32)
        if case % 4 >= 2:
            pos = np.cumsum(rng.integers(0, 30, L)).astype(np.int64)
            if chrom is not None:
                for a, e in T.blocks(chrom, L):
                    pos[a:e] -= pos[a] - int(rng.integers(0, 5))
        pairs = None
        if case % 5 == 0:                                # a list in any order, with duplicates
            allp = [(i, j) for i in range(n) for j in range(i + 1, n)]
            pairs = [allp[int(k)] for k in rng.integers(0, len(allp), int(rng.integers(1, 2 * len(allp) + 1)))]
        prm = dict(mode=1 + case % 2 if case % 7 else 2, min_snp=int(rng.integers(1, 6)), merge_min=int(rng.integers(0, 6)),
                   min_len=int(rng.choice([0, 0, 20])), max_gap=int(rng.choice([0, 12, 25])))
        want = T.ibd_loops(g, called, pairs, chrom, pos, **prm)
        got = r_api.ibd_host(g, called, None if pairs is None else np.asarray(pairs), chrom, pos, **prm)
        same(got, want, (case, prm))
        some += want[1].shape[0]
        merged += int((want[1][:, 4] > 0).sum())
    assert some > 1000 and merged > 100


def pair_of(breaks, L, uncalled=()):
    """Two individuals, all hom A1, with opposite homozygotes (a break in both modes) at `breaks`; at `uncalled` individual 1 would be a
    break but is not called."""
    g = -np.ones((L, 2), dtype=np.int8)
    called = np.ones((L, 2), dtype=bool)
    for m in list(breaks) + list(uncalled):
        g[m, 1] = 1
    for m in uncalled:
        called[m, 1] = False
    return g, called


@pytest.mark.parametrize("mode", (1, 2))
def test_hand_cases_at_every_threshold(mode):
    from eagleeverything_amd import r_api

    def run(g, called=None, chrom=None, pos=None, **prm):
        got = r_api.ibd_host(g, called, None, chrom, pos, mode=mode, **prm)
        same(got, T.ibd_loops(g, called, None, chrom, pos, mode=mode, **prm), prm)
        return got[1][:, 2:6].tolist()
    # a run of exactly min_snp and of min_snp - 1: 0 .. 9 | break 10 | 11 .. 19
    g, _ = pair_of([10], 20)
    assert run(g, min_snp=10, merge_min=0) == [[0, 9, 0, 0]]
    assert run(g, min_snp=9, merge_min=0) == [[0, 9, 0, 0], [11, 19, 0, 0]]
    assert run(g, min_snp=11, merge_min=0) == []
    # a neighbour run of exactly merge_min and of merge_min - 1
    assert run(g, min_snp=1, merge_min=9) == [[0, 19, 1, 0]]
    assert run(g, min_snp=1, merge_min=10) == [[0, 9, 0, 0], [11, 19, 0, 0]]
    assert run(g, min_snp=20, merge_min=9) == [[0, 19, 1, 0]] and run(g, min_snp=21, merge_min=9) == []
    # three runs of 10, 4 and 10: the ineligible middle run is a chain of its own and keeps its neighbours apart
    g, _ = pair_of([10, 15], 26)
    assert run(g, min_snp=1, merge_min=5) == [[0, 9, 0, 0], [11, 14, 0, 0], [16, 25, 0, 0]]
    assert run(g, min_snp=1, merge_min=4) == [[0, 25, 2, 0]]
    # two adjacent breaks end a chain
    g, _ = pair_of([10, 11], 22)
    assert run(g, min_snp=1, merge_min=1) == [[0, 9, 0, 0], [12, 21, 0, 0]]
    # a cut between two eligible runs: a block bound, and a gap with the break right before / after it
    g, _ = pair_of([], 20)
    chrom = np.repeat([4, 9], 10).astype(np.int32)
    assert run(g, chrom=chrom, min_snp=1, merge_min=1) == [[0, 9, 0, 0], [10, 19, 0, 1]]
    pos = np.arange(20, dtype=np.int64) * 10
    pos[10:] += 100
    g, _ = pair_of([9], 20)
    assert run(g, pos=pos, min_snp=1, merge_min=1, max_gap=109) == [[0, 8, 0, 0], [10, 19, 0, 0]]
    assert run(g, pos=pos, min_snp=1, merge_min=1, max_gap=110) == [[0, 19, 1, 0]]
    assert run(g, pos=pos, min_snp=1, merge_min=1, max_gap=110, min_len=290) == [[0, 19, 1, 0]]
    assert run(g, pos=pos, min_snp=1, merge_min=1, max_gap=110, min_len=291) == []
    g, _ = pair_of([10], 20)
    assert run(g, pos=pos, min_snp=1, merge_min=1, max_gap=109) == [[0, 9, 0, 0], [11, 19, 0, 0]]
    # a break on the first and last marker of a block
    g, _ = pair_of([0, 9, 10, 19], 20)
    assert run(g, chrom=chrom, min_snp=1, merge_min=1) == [[1, 8, 0, 0], [11, 18, 0, 1]]
    # a not-called marker at a would-be break: no break there
    g, called = pair_of([], 20, uncalled=[10])
    assert run(g, called, min_snp=1, merge_min=0) == [[0, 19, 0, 0]]
    assert run(g, None, min_snp=1, merge_min=0) == [[0, 9, 0, 0], [11, 19, 0, 0]]
    # a single marker
    assert run(-np.ones((1, 2), dtype=np.int8), min_snp=1, merge_min=0) == [[0, 0, 0, 0]]
    assert run(np.array([[-1, 1]], dtype=np.int8), min_snp=1, merge_min=0) == []


def test_modes_differ_where_a_het_meets_a_homozygote():
    from eagleeverything_amd import r_api
    g = -np.ones((12, 2), dtype=np.int8)
    g[5, 1] = 0                                          # het against hom: equal no more, but no opposite homozygotes
    assert r_api.ibd_host(g, mode="ibs1", min_snp=1, merge_min=0)[1][:, 2:4].tolist() == [[0, 11]]
    assert r_api.ibd_host(g, mode="ibs2", min_snp=1, merge_min=0)[1][:, 2:4].tolist() == [[0, 4], [6, 11]]
    with pytest.raises(ValueError):
        r_api.ibd_host(g, mode=3)
    with pytest.raises(ValueError):
        r_api.ibd_host(g, pairs=[[1, 0]])
    with pytest.raises(ValueError):
        r_api.ibd_host(g, pos=np.arange(12)[::-1])


def test_incidence_shared_and_kinship():
    from eagleeverything_amd import r_api
    L = 600
    g, _ = T.mosaic(6, L, 3, seed=4)
    g[:, 5] = g[:, 0]                                    # a duplicate pair
    chrom = np.repeat([1, 2, 3], 200).astype(np.int32)
    pos = np.tile(np.arange(200, dtype=np.int64) * 1000, 3)
    out = {}
    for mode in ("ibs1", "ibs2"):
        tab, seg = r_api.ibd_host(g, None, None, chrom, pos, mode=mode, min_snp=10, merge_min=5)
        assert seg.shape[0] > 0
        inc = r_api.ibd_incidence(seg, L)
        want = np.zeros(L, dtype=np.int64)
        for row in seg.tolist():
            for m in range(row[2], row[3] + 1):
                want[m] += 1
        assert np.array_equal(inc, want) and inc.max() >= 1
        res = r_api.ibd_summary(r_api.ibd_all_pairs(6), tab, seg, L, chrom, pos)
        assert np.array_equal(res["shared"], tab[:, 2] / np.float64(3 * 199 * 1000))
        assert np.array_equal(res["segments"]["length"], pos[seg[:, 3]] - pos[seg[:, 2]]) and np.array_equal(res["ibd_incidence"], inc)
        k = 4                                            # the ordinal of (0, 5) among the pairs of 6
        assert res["pairs"][k].tolist() == [0, 5] and tab[k].tolist() == [3, 600, 3 * 199000, 199000] and res["shared"][k] == 1.0
        out[mode] = res
    kin = r_api.ibd_kinship(out["ibs1"], out["ibs2"])
    assert kin[4] == 0.5 and np.all(kin <= 0.5) and np.array_equal(kin, (out["ibs1"]["shared"] + out["ibs2"]["shared"]) / 4.0)
    assert np.all(out["ibs2"]["total_length"] <= out["ibs1"]["total_length"])        # an ibs2 run lies inside an ibs1 run
    with pytest.raises(ValueError):
        r_api.ibd_incidence(np.array([[0, 1, 5, L, 0, 0]]), L)
    with pytest.raises(ValueError):
        r_api.ibd_kinship(np.zeros(3), np.zeros(4))


def test_the_mosaic_panel_gives_segments_at_the_thresholds_the_gpu_tests_use():
    g, _ = T.mosaic(5, 700, 3, seed=1)
    chrom = np.repeat([1, 2, 3], [250, 250, 200]).astype(np.int32)
    for (min_snp, merge_min) in ((3, 0), (30, 10), (20, 1)):
        for mode in (1, 2):
            tab, seg = T.ibd_loops(g, None, None, chrom, None, mode=mode, min_snp=min_snp, merge_min=merge_min)
            assert seg.shape[0] >= 1 and int(tab[:, 0].sum()) == seg.shape[0]
            if merge_min:
                assert (seg[:, 4] >= 1).any()
