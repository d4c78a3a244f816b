"""CPU: r_api.roh_host, the numpy restatement of the runs of homozygosity (include/eagle_hip.h section 1b'''vi), against the plain loops
of tests/roh_truth.py on random small cases, every equality case of the segment filters and of the flag threshold one side each way,
the planted panel's properties, roh_incidence against a per-marker loop, and the argument refusals.  Every comparison is ==."""
import numpy as np
import pytest

import roh_truth as T
from eagleeverything_amd import r_api


def same(a, b):
    assert a[0].dtype == np.int64 and a[1].dtype == np.int32 and a[1].ndim == 2 and a[1].shape[1] == 6
    assert np.array_equal(a[0], b[0]), (a[0], b[0])
    assert np.array_equal(a[1], b[1]), (a[1], b[1])


def test_roh_host_equals_the_loops_on_random_small_cases():
    rng = np.random.default_rng(20261)
    cases = 0
    for trial in range(320):
        L, n, w = int(rng.integers(1, 41)), int(rng.integers(1, 5)), int(rng.integers(1, 10))
        het_rate = float(rng.choice([0.05, 0.2, 0.5]))
        cl = (rng.random((L, n)) < het_rate).astype(np.uint8)
        if trial % 2:
            cl[rng.random((L, n)) < 0.1] = 2
        chrom = None if trial % 3 == 0 else np.sort(rng.integers(0, int(rng.integers(1, 5)), L)).astype(np.int32)[::int(rng.choice([-1, 1]))]
        pos = None
        if trial % 4 >= 2:
            pos = np.cumsum(rng.integers(0, 6, L)).astype(np.int64)
            if chrom is not None:                        # restart in every block: positions are free across block edges
                for a, e in T.blocks(chrom, L):
                    pos[a:e] -= pos[a] - int(rng.integers(0, 4))
        p = dict(w=w, win_het=int(rng.integers(0, 3)), win_miss=int(rng.integers(0, 3)), thr16=int(rng.choice([0, 1, 3277, 32768, 50000, 65536])),
                 min_snp=int(rng.integers(1, 6)), min_len=int(rng.integers(0, 8)), max_gap=int(rng.choice([0, 1, 2, 4])),
                 max_density=int(rng.choice([0, 1, 2, 3])), max_het=int(rng.choice([-1, 0, 1, 2])))
        same(r_api.roh_host(cl, chrom, pos, **p), T.roh_loops(cl, chrom, pos, **p))
        cases += 1
    assert cases >= 300


def one(classes, pos=None, chrom=None, **p):
    base = dict(w=1, win_het=0, win_miss=0, thr16=65536, min_snp=1, min_len=0, max_gap=0, max_density=0, max_het=-1)
    base.update(p)
    cl = np.asarray(classes, dtype=np.uint8).reshape(-1, 1)
    got = r_api.roh_host(cl, chrom, pos, **base)
    same(got, T.roh_loops(cl, chrom, pos, **base))
    return got[1][:, 1:5].tolist()


def test_every_equality_case_of_the_segment_filters():
    run5 = [1, 0, 0, 0, 0, 0, 1]                      # w = 1: a marker is flagged iff it is hom; one run, markers 1 .. 5
    assert one(run5, min_snp=5) == [[1, 5, 0, 0]] and one(run5, min_snp=6) == []                           # nsnp at min_snp and min_snp - 1
    pos = [0, 10, 11, 12, 13, 30, 31]                 # len = 20
    assert one(run5, pos, min_len=20) == [[1, 5, 0, 0]] and one(run5, pos, min_len=21) == []              # len at min_len and min_len - 1
    assert one(run5, pos, max_density=4) == [[1, 5, 0, 0]]                                                # len = 20 = 4 * 5
    assert one(run5, [0, 10, 11, 12, 13, 31, 32], max_density=4) == []                                    # len = 21: one more
    # nhet inside a run needs a window that tolerates a het: w = 2, win_het = 1, thr16 = 0 flags every marker with one homozygous window
    withhet = [0, 0, 1, 0, 0, 1, 0, 0]
    base = dict(w=2, win_het=1, thr16=0)
    assert one(withhet, **base, max_het=2) == [[0, 7, 2, 0]] and one(withhet, **base, max_het=1) == []    # nhet at max_het and max_het + 1
    assert one(withhet, **base, max_het=-1) == [[0, 7, 2, 0]]
    # gaps
    run = [0, 0, 0, 0]
    assert one(run, [0, 5, 10, 15], max_gap=5) == [[0, 3, 0, 0]]                                           # a gap equal to max_gap: no break
    assert one(run, [0, 5, 11, 16], max_gap=5) == [[0, 1, 0, 0], [2, 3, 0, 0]]                             # max_gap + 1: a break
    assert one(run, [0, 5, 11, 16], max_gap=0) == [[0, 3, 0, 0]]                                           # 0: no gap rule
    # missing calls are counted in nmiss, not in nhet
    assert one([0, 2, 0], w=1, win_miss=1) == [[0, 2, 0, 1]] and one([0, 2, 0], w=1, win_miss=0) == [[0, 0, 0, 0], [2, 2, 0, 0]]


def test_the_flag_threshold_at_equality():
    # w = 2, one block of three markers, classes hom hom het: windows [0, 1] homozygous, [1, 2] not.  Marker 1: cover = 2, hom = 1.
    cl = np.array([[0], [0], [1]], dtype=np.uint8)
    base = dict(w=2, win_het=0, win_miss=0, min_snp=1)
    at = r_api.roh_host(cl, **base, thr16=32768)[1]
    over = r_api.roh_host(cl, **base, thr16=32769)[1]
    assert at[:, 1:3].tolist() == [[0, 1]] and over[:, 1:3].tolist() == [[0, 0]]
    f = T.flags_loops(cl, None, dict(T.DEFAULTS, **base, thr16=32768))[:, 0].tolist()
    assert f == [True, True, False] and T.flags_loops(cl, None, dict(T.DEFAULTS, **base, thr16=32769))[:, 0].tolist() == [True, False, False]
    # hom >= 1 is required even at thr16 = 0, and a block shorter than w has no flagged marker
    assert r_api.roh_host(np.ones((4, 1), dtype=np.uint8), **base, thr16=0)[1].shape == (0, 6)
    assert r_api.roh_host(np.zeros((3, 2), dtype=np.uint8), w=4, min_snp=1)[1].shape == (0, 6)
    assert r_api.roh_host(np.zeros((4, 2), dtype=np.uint8), w=4, min_snp=1)[1][:, :3].tolist() == [[0, 0, 3], [1, 0, 3]]


PLANTED = [(0, 40, 219), (0, 300, 420), (2, 0, 130), (3, 480, 599), (5, 250, 380)]


def test_planted_panel():
    n, L = 8, 600
    cl = T.planted_panel(n, L, 7, PLANTED)
    chrom = np.repeat([1, 2], [300, 300]).astype(np.int32)
    pos = np.concatenate([np.arange(300), np.arange(300)]).astype(np.int64) * 1000
    p = dict(w=20, win_het=1, win_miss=0, thr16=3277, min_snp=50, min_len=40000)
    ind, seg = r_api.roh_host(cl, chrom, pos, **p)
    same((ind, seg), T.roh_loops(cl, chrom, pos, **p))
    for i, s, e in PLANTED:
        parts = [(max(s, a), min(e, b - 1)) for a, b in ((0, 300), (300, 600)) if max(s, a) <= min(e, b - 1)]
        for ps, pe in parts:                        # a planted stretch is cut at the chromosome edge; a part of at least min_snp markers is found
            if pe - ps + 1 >= 50:
                assert np.any((seg[:, 0] == i) & (seg[:, 1] <= ps) & (seg[:, 2] >= pe)), (i, ps, pe)
    res = r_api.roh_summary(ind, seg, L, chrom, pos)
    planted = sorted({i for i, _, _ in PLANTED})
    others = [i for i in range(n) if i not in planted]
    assert res["F_ROH"][planted].min() > res["F_ROH"][others].max()
    assert np.array_equal(res["F_ROH"], ind[:, 2] / np.float64(2 * 299000))
    inc = np.zeros(L, dtype=np.int64)
    for m in range(L):
        inc[m] = sum(1 for r in seg if r[1] <= m <= r[2])
    assert np.array_equal(r_api.roh_incidence(seg, L), inc) and np.array_equal(res["incidence"], inc) and inc.max() >= 1
    assert np.array_equal(res["segments"]["length"], pos[seg[:, 2]] - pos[seg[:, 1]]) and np.array_equal(res["nseg"], ind[:, 0])


def test_classes_helpers():
    Mt8 = np.array([[-1, 0, 1], [0, 0, -1]], dtype=np.int8)
    assert r_api.roh_classes_mt8(Mt8).tolist() == [[0, 1, 0], [1, 1, 0]]
    codes = np.array([[0, 1, 2, 3]], dtype=np.uint8)
    assert r_api.roh_classes_bed(codes).tolist() == [[0, 2, 1, 0]]
    cl = T.planted_panel(5, 30, 1, [(1, 3, 20)], miss_rate=0.1)
    assert np.array_equal(r_api.roh_classes_bed(T.bed_codes_of_classes(cl)), cl)
    cl2 = np.minimum(cl, 1)
    assert np.array_equal(r_api.roh_classes_mt8(T.mt8_of_classes(cl2)), cl2)


def test_wrong_arguments_raise():
    cl = np.zeros((6, 2), dtype=np.uint8)
    for kw in (dict(w=0), dict(w=65), dict(thr16=65537), dict(min_snp=0), dict(max_density=-1), dict(win_het=-1), dict(nope=1)):
        with pytest.raises(ValueError):
            r_api.roh_host(cl, **kw)
    with pytest.raises(ValueError):
        r_api.roh_host(cl, chrom=[1, 1])
    with pytest.raises(ValueError):
        r_api.roh_host(cl, pos=[1, 2, 3, 2, 5, 6])
    with pytest.raises(ValueError):
        r_api.roh_host(np.full((6, 2), 3, dtype=np.uint8))
    with pytest.raises(ValueError):
        r_api.roh_host(np.zeros(6, dtype=np.uint8))
    r_api.roh_host(cl, chrom=[1, 1, 1, 2, 2, 2], pos=[1, 2, 3, 1, 2, 3], w=2, min_snp=1)        # going down across a block edge is fine
    with pytest.raises(ValueError):
        r_api.roh_incidence(np.array([[0, 2, 7, 0, 0, 0]]), 6)
    with pytest.raises(ValueError):
        r_api.roh_thr16(1.5)
    geno = {"dim_of_ascii_M": [4, 6], "asciifileMt": "/nonexistent/Mt.ascii"}
    for kw in (dict(), dict(min_kb=None), dict(min_kb=None, max_density_kb=None), dict(min_kb=None, max_gap_kb=None)):
        with pytest.raises(ValueError, match="needs a map"):
            r_api.ROH(geno, **kw)                   # without a map the three kb arguments must be None
    with pytest.raises(ValueError):
        r_api.ROH(geno, include=[0, 1])             # include= needs bed=
