"""Runs of homozygosity on the GPU from the ingested panel: eagle_roh (k_roh_flags<image>, k_roh_segments) and r_api.ROH on top.

The device's tables are compared with r_api.roh_host(r_api.roh_classes_mt8(...)) -- the numpy restatement that tests/test_roh_host.py
pins to plain loops of the definitions (include/eagle_hip.h section 1b'''vi).  Everything is integers: every comparison is ==."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import roh_truth as T

pytestmark = pytest.mark.gpu

CHUNK = 1024                                             # EAGLE_ROH_CHUNK
NS = (1, 63, 64, 65, 257)
WS = (1, 2, 50, 63, 64)


def small_blocks(w):
    return [b for b in (w - 1, w, w + 1, 2 * w - 1, 2 * w) if b > 0]


def layout(w, kind, d=0):
    """Block lengths.  Both kinds start with blocks of w - 1, w, w + 1, 2 w - 1 and 2 w markers.  "edges": block bounds at CHUNK + d and
    2 CHUNK + d, then a short last block.  "long": one block from there across CHUNK and 2 CHUNK to 2 CHUNK + w + 4."""
    sm = small_blocks(w)
    S = sum(sm)
    if kind == "edges":
        return sm + [CHUNK + d - S, CHUNK, 2 * w + 5]
    return sm + [2 * CHUNK + w + 4 - S]


def chrom_of(lengths):
    return np.repeat(np.arange(len(lengths)) % 3 + 5, lengths).astype(np.int32)       # 5, 6, 7, 5, ...: a chromosome code comes back


def pos_of(lengths, seed):
    """Base pairs: steps of 1 .. 2,000, every 97th step 50,000; every block starts again near 0 (positions are free across block edges)."""
    rng = np.random.default_rng(seed)
    L = int(sum(lengths))
    step = rng.integers(1, 2001, L).astype(np.int64)
    step[::97] = 50000
    pos = np.cumsum(step)
    a = 0
    for b in lengths:
        pos[a:a + b] -= pos[a] - int(rng.integers(0, 1000))
        a += b
    return pos


def background(n, L, seed):
    """Classes 0 / 1 with a het rate per individual between 0.005 and 0.3: every window rule from w = 1 to 64 finds something."""
    rng = np.random.default_rng(seed)
    rate = rng.choice([0.005, 0.02, 0.05, 0.3], n)
    return (rng.random((L, n)) < rate[None, :]).astype(np.uint8)


VARIANTS = (dict(win_het=1, thr16=3277, min_snp=3),
            dict(win_het=0, thr16=32768, min_snp=2, min_len=3000, max_gap=20000, max_density=1500, max_het=1),
            dict(win_het=2, thr16=0, min_snp=1, max_gap=49999, max_het=0))


def same(got, want, what):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[0].shape == want[0].shape and got[1].ndim == 2, what
    assert np.array_equal(got[0], want[0]), (what, "ind", np.flatnonzero((got[0] != want[0]).any(axis=1))[:10])
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), (what, "seg", got[1][:5], want[1][:5])


def write_panel(tmp_path, cl, name="Mt.ascii"):
    from eagleeverything_amd import synth
    path = str(tmp_path / name)
    synth.write_ascii(path, T.mt8_of_classes(cl, seed=3))
    return path


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("n", NS)
def test_gpu_roh_equals_host_at_block_and_chunk_edges(tmp_path, n, w):
    from eagleeverything_amd import r_api, rcpp_api
    rcpp_api.drop_cache()
    some = 0
    for k, (kind, d) in enumerate((("edges", -1), ("edges", 0), ("edges", 1), ("long", 0))):
        lengths = layout(w, kind, d)
        L = sum(lengths)
        cl = background(n, L, seed=1000 * n + 10 * w + k)
        chrom, pos = chrom_of(lengths), pos_of(lengths, seed=k)
        Mt = write_panel(tmp_path, cl, "Mt%d.ascii" % k)
        for v, prm in enumerate(VARIANTS if kind == "long" else VARIANTS[:1]):
            want = r_api.roh_host(cl, chrom, pos, w=w, **prm)
            got = rcpp_api.roh(Mt, (n, L), chrom, pos, w=w, **prm)
            same(got, want, (n, w, kind, d, v))
            some += want[1].shape[0]
        if kind == "long":                               # no map: one block, pos = the marker index
            want = r_api.roh_host(cl, w=w, win_het=1, min_snp=4, max_density=1)
            same(rcpp_api.roh(Mt, (n, L), w=w, win_het=1, min_snp=4, max_density=1), want, (n, w, "no map"))
            assert np.all(want[1][:, 5] == 0)
    assert some > 0
    rcpp_api.drop_cache()


@functools.lru_cache(maxsize=None)
def planted():
    """n = 257, w = 50, the "long" layout.  Individuals: 2 all hom; 3 all het; 4, 5, 6 all hom with one het at CHUNK - 1, CHUNK, CHUNK + 1;
    7 hom on the first 80 markers of the long block and het elsewhere; 8 hom on its last 80; 0 = 256 and 1 = 65 (identical columns in
    different waves of both kernels)."""
    n, w = 257, 50
    lengths = layout(w, "long")
    L = sum(lengths)
    cl = background(n, L, seed=99)
    a = L - lengths[-1]
    cl[:, 2] = 0
    cl[:, 3] = 1
    for i, m in ((4, CHUNK - 1), (5, CHUNK), (6, CHUNK + 1)):
        cl[:, i] = 0
        cl[m, i] = 1
    cl[:, 7] = 1
    cl[a:a + 80, 7] = 0
    cl[:, 8] = 1
    cl[L - 80:, 8] = 0
    cl[:, 256] = cl[:, 0]
    cl[:, 65] = cl[:, 1]
    chrom = chrom_of(lengths)
    pos = np.arange(L, dtype=np.int64) * 100
    pos[a + 700:] += 5000                                # one gap of 5,100 inside the long block
    cl.setflags(write=False)
    return n, w, lengths, L, a, cl, chrom, pos


def test_gpu_roh_planted_cases(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    n, w, lengths, L, a, cl, chrom, pos = planted()
    Mt = write_panel(tmp_path, cl)
    rcpp_api.drop_cache()
    for win_het in (0, 1):
        for max_gap in (0, 5099, 5100):
            prm = dict(w=w, win_het=win_het, thr16=0, min_snp=10, max_gap=max_gap)       # thr16 = 0: flagged iff one window is homozygous
            want = r_api.roh_host(cl, chrom, pos, **prm)
            ind, seg = rcpp_api.roh(Mt, (n, L), chrom, pos, **prm)
            same((ind, seg), want, (win_het, max_gap))
            rows = lambda i: seg[seg[:, 0] == i][:, 1:6].tolist()                        # noqa: E731
            full = [[s, s + b - 1, 0, 0, k] for k, (s, b) in enumerate(zip(np.cumsum([0] + lengths[:-1]).tolist(), lengths)) if b >= w]
            if max_gap == 5099:                          # the gap of 5,100 splits the long block's run
                full = full[:-1] + [[a, a + 699, 0, 0, len(lengths) - 1], [a + 700, L - 1, 0, 0, len(lengths) - 1]]
            assert rows(2) == full                       # all hom: one run per block of at least w markers, split by the gap
            assert rows(3) == [] and ind[3].tolist() == [0, 0, 0, 0]                     # all het
            for i, m in ((4, CHUNK - 1), (5, CHUNK), (6, CHUNK + 1)):
                r = [x for x in rows(i) if x[4] == len(lengths) - 1]
                if win_het == 1:                         # the het is tolerated: it lies inside a run and is counted
                    assert any(x[0] < m < x[1] and x[2] == 1 for x in r), (i, r)
                else:                                    # no window over the het is homozygous: the runs stop beside it
                    assert any(x[1] == m - 1 for x in r) and any(x[0] == m + 1 for x in r) and all(x[2] == 0 for x in r), (i, r)
            assert [x[:2] for x in rows(7)] == [[a, a + 79 + win_het]] and [x[:2] for x in rows(8)] == [[L - 80 - win_het, L - 1]]
            assert rows(256) == rows(0) and rows(65) == rows(1) and np.array_equal(ind[256], ind[0]) and np.array_equal(ind[65], ind[1])
    rcpp_api.drop_cache()


def test_gpu_roh_capacity(tmp_path):
    """seg_cap = 0 returns the totals, seg_cap = total fills the rows, seg_cap = total - 1 leaves the buffer untouched."""
    from eagleeverything_amd import _lib, r_api, rcpp_api
    n, w, lengths, L, a, cl, chrom, pos = planted()
    Mt = write_panel(tmp_path, cl)
    rcpp_api.drop_cache()
    want_ind, want_seg = r_api.roh_host(cl, chrom, pos, w=w, min_snp=10)
    total = want_seg.shape[0]
    assert total > 10
    lib, ctx = _lib.load(), rcpp_api.context(0)
    p = dict(rcpp_api.ROH_DEFAULTS, w=w, min_snp=10)
    prm = _lib.RohParams(*[p[f] for f in rcpp_api._ROH_FIELDS])
    dims = (C.c_long * 2)(n, L)
    ch, ps = np.ascontiguousarray(chrom), np.ascontiguousarray(pos)

    def call(seg, cap):
        ind, got = np.zeros((n, 4), dtype=np.int64), C.c_long(-1)
        rc = lib.eagle_roh(ctx, os.fsencode(Mt), dims, ch.ctypes.data_as(C.POINTER(C.c_int32)), ps.ctypes.data_as(C.POINTER(C.c_int64)),
                           C.addressof(prm), 8.0, ind.ctypes.data_as(C.POINTER(C.c_int64)),
                           seg.ctypes.data_as(C.POINTER(C.c_int32)) if seg is not None else None, cap, C.byref(got))
        assert rc == 0
        return ind, got.value
    ind, got = call(None, 0)
    assert got == total and np.array_equal(ind, want_ind)
    seg = np.full((total + 1, 6), -7, dtype=np.int32)
    ind, got = call(seg, total)
    assert got == total and np.array_equal(ind, want_ind) and np.array_equal(seg[:total], want_seg) and np.all(seg[total] == -7)
    seg = np.full((total, 6), -7, dtype=np.int32)
    ind, got = call(seg, total - 1)
    assert got == total and np.array_equal(ind, want_ind) and np.all(seg == -7)
    ind, seg = rcpp_api.roh(Mt, (n, L), chrom, pos, w=w, min_snp=10, seg_cap=1)          # the wrapper calls once more
    assert np.array_equal(ind, want_ind) and np.array_equal(seg, want_seg)
    rcpp_api.drop_cache()


def test_gpu_roh_streamed_equals_resident(tmp_path, monkeypatch):
    from eagleeverything_amd import r_api, rcpp_api
    n, L = 256, 5120
    cl = background(n, L, seed=5)
    lengths = [1700, 90, 2, 1, 255, 1536, 1536]          # bounds around the rows where row windows of 1,792 rows and their cores end
    assert sum(lengths) == L
    chrom, pos = chrom_of(lengths), pos_of(lengths, seed=8)
    for m in (1600, 1665, 1666, 1728, 1729, 1791, 1792, 3331, 3332, 3395, 4997):
        cl[m - 70:m + 70, 7::16] = 0                     # segments across those rows
        cl[m, 7::32] = 1
    Mt = write_panel(tmp_path, cl)
    cases = [dict(w=64, win_het=1, min_snp=20, max_gap=30000), dict(w=50, win_het=0, thr16=32768, min_snp=5), dict(w=1, min_snp=3)]
    rcpp_api.drop_cache()
    resident = []
    for prm in cases:
        want = r_api.roh_host(cl, chrom, pos, **prm)
        resident.append(rcpp_api.roh(Mt, (n, L), chrom, pos, **prm))
        same(resident[-1], want, ("resident", prm["w"]))
        assert want[1].shape[0] >= 16
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.001")                             # 1 MB: the image goes in several row windows
    for prm, res in zip(cases, resident):
        same(rcpp_api.roh(Mt, (n, L), chrom, pos, **prm), res, ("streamed", prm["w"]))
    rcpp_api.drop_cache()


def test_gpu_roh_view_alias_gives_the_kept_individuals(tmp_path):
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    n, L, w = 70, 300, 20
    cl = background(n, L, seed=12)
    Mt8 = T.mt8_of_classes(cl, seed=4)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    drop = np.array([1, 2, 33, 64, 65, 70])              # 1-based, as AM's indxNA
    kept = np.setdiff1d(np.arange(n), drop - 1)
    sub = am.reshape_geno(geno, drop, view=True)
    nk = n - drop.size
    assert list(sub["dim_of_ascii_M"]) == [nk, L]
    own = str(tmp_path / "own.ascii")
    synth.write_ascii(own, Mt8[:, kept])
    prm = dict(w=w, win_het=1, min_snp=5)
    got = rcpp_api.roh(sub["asciifileMt"], (nk, L), **prm)
    same(got, rcpp_api.roh(own, (nk, L), **prm), "view against the subset's own file")
    same(got, r_api.roh_host(cl[:, kept], **prm), "view against the host")
    assert got[1].shape[0] > 0
    rcpp_api.drop_cache()


def test_gpu_ROH_with_and_without_a_map(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L = 65, 1300
    cl = T.planted_panel(n, L, 3, [(0, 100, 400), (5, 600, 1299), (64, 0, 250), (64, 1040, 1200)], het_rate=0.3)
    geno = synth.write_geno_pair(str(tmp_path), T.mt8_of_classes(cl, seed=6))
    rcpp_api.drop_cache()
    # without a map: one block, lengths in markers, the kb arguments must be None
    res = r_api.ROH(geno, min_kb=None, max_density_kb=None, max_gap_kb=None)
    ind, seg = r_api.roh_host(cl, w=50, win_het=1, win_miss=5, thr16=r_api.roh_thr16(0.05), min_snp=100)
    assert np.array_equal(res["ind"], ind) and np.array_equal(res["seg"], seg) and seg.shape[0] >= 4
    assert np.array_equal(res["F_ROH"], ind[:, 2] / np.float64(L - 1)) and res["F_ROH"][5] > 0.5 and res["F_ROH"][1] == 0.0
    assert np.array_equal(res["incidence"], r_api.roh_incidence(seg, L)) and res["incidence"][1100] == 2
    with pytest.raises(ValueError):
        r_api.ROH(geno)
    # with a map: two chromosomes, base pairs, the kb filters converted
    chrom = (np.arange(L) >= 1024).astype(np.int32)
    pos = np.where(chrom == 0, np.arange(L), np.arange(L) - 1024).astype(np.int64) * 4000 + 17
    map = {"SNP": ["m%d" % i for i in range(L)], "Chr": ["chrB" if c else "chrA" for c in chrom], "Pos": [int(p) for p in pos]}
    res = r_api.ROH(geno, map=map, min_snp=60, min_kb=300, max_density_kb=4, max_gap_kb=4, max_het=3)
    want = r_api.roh_host(cl, chrom, pos, w=50, win_het=1, win_miss=5, thr16=3277, min_snp=60, min_len=300000, max_density=4000, max_gap=4000,
                          max_het=3)
    assert np.array_equal(res["ind"], want[0]) and np.array_equal(res["seg"], want[1]) and want[1].shape[0] >= 4
    ref = r_api.roh_summary(want[0], want[1], L, chrom, pos)
    assert np.array_equal(res["F_ROH"], want[0][:, 2] / np.float64(1023 * 4000 + 275 * 4000))
    for k in ref["segments"]:
        assert np.array_equal(res["segments"][k], ref["segments"][k]), k
    assert set(res["segments"]["block"].tolist()) == {0, 1}                              # individual 5's stretch is cut at the chromosome edge
    assert r_api.ROH(geno, map=map, min_snp=60, min_kb=300, max_density_kb=3.9, max_gap_kb=4)["seg"].shape[0] == 0       # markers 4 kb apart: too sparse
    rcpp_api.drop_cache()
