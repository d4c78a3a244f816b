"""Pairwise IBD-type segments on the GPU from the ingested panel: eagle_ibd (k_ibd_planes_i8, k_ibd_walk) on M.ascii.

The device's tables are compared with r_api.ibd_host -- the numpy restatement that tests/test_ibd_host.py pins to plain loops of the
definitions (include/eagle_hip.h section 1b'''vii).  Everything is integers: every comparison is ==."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import ibd_truth as T
from test_gpu_roh import chrom_of, pos_of

pytestmark = pytest.mark.gpu

NS = (2, 3, 64, 65, 129)                                 # one pair, and the edges of the 64-lane pair tiles
LS = (1, 63, 64, 65, 127, 128, 129)
LENGTHS = (639, 641, 641, 179)                           # block bounds at 64 k - 1, 64 k and 64 k + 1: 639, 1280, 1921
LM = sum(LENGTHS)
# (min_snp, merge_min, min_len, max_gap); pos as test_gpu_roh.py builds it: steps of 1 .. 2,000, every 97th step 50,000
VARIANTS = (dict(min_snp=3, merge_min=0, min_len=0, max_gap=0),
            dict(min_snp=30, merge_min=10, min_len=3000, max_gap=20000),
            dict(min_snp=20, merge_min=1, min_len=0, max_gap=49999))
SEQ_AT = 1350                                            # where the planted run lengths start, inside the block [1280, 1921)
SEQ_RUNS = (30, 29, 10, 9, 20, 19, 3, 2)                 # min_snp and min_snp - 1, merge_min and merge_min - 1 of the variants


def same(got, want, what):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[0].shape == want[0].shape and got[1].ndim == 2, what
    assert np.array_equal(got[0], want[0]), (what, "pair", np.flatnonzero((got[0] != want[0]).any(axis=1))[:10])
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), (what, "seg", got[1][:5], want[1][:5])


def write_M(tmp_path, g, name="M.ascii"):
    """The individual-major file of the marker-major image g (L, n)."""
    from eagleeverything_amd import synth
    return synth.write_ascii(str(tmp_path / name), np.ascontiguousarray(g.T))


def planted_markers():
    """Where the planted pairs get a break: bits 0 and 63 of the words on both sides of every block bound (among them the first and the last
    marker of a block), then single breaks around runs of SEQ_RUNS markers, two adjacent breaks, a run of 12 and a last break.
    -> (breaks, the marker whose break is not called in the .bed tests)."""
    out = []
    for bound in np.cumsum(LENGTHS)[:-1].tolist():
        w = bound // 64
        out += [64 * (w - 1), 64 * w - 1, 64 * w, 64 * w + 63]
    cur = SEQ_AT
    out.append(cur)
    cur += 1
    for ln in SEQ_RUNS:
        cur += ln
        out.append(cur)
        cur += 1
    out.append(cur)                                      # two breaks in a row
    cur += 1 + 12
    out.append(cur)
    hidden = cur + 40                                    # a would-be break that is not called (.bed route); a plain break on the image
    return sorted(set(out)), hidden


def plant(g, called, a, b, hide):
    """Individual b becomes a copy of a, with opposite homozygotes at the planted markers."""
    g[:, b] = g[:, a]
    called[:, b] = called[:, a]
    brk, hidden = planted_markers()
    for m in brk + [hidden]:
        if g[m, a] == 0:
            g[m, a] = -1
        g[m, b] = -g[m, a]
        called[m, a] = called[m, b] = True
    if hide:
        called[hidden, b] = False


@functools.lru_cache(maxsize=None)
def mosaic_panel(n, miss=0.0):
    """The mosaic panel of LM markers with the hand cases planted in pair (0, 1) and in the last pair -> (g, called, chrom, pos), read-only."""
    g, called = T.mosaic(n, LM, 3, seed=100 + n, miss=miss)
    plant(g, called, 0, 1, miss > 0)
    if n > 2:
        plant(g, called, n - 2, n - 1, miss > 0)
    g[~called] = 0
    chrom, pos = chrom_of(list(LENGTHS)), pos_of(list(LENGTHS), seed=n)
    for x in (g, called, chrom, pos):
        x.setflags(write=False)
    return g, called, chrom, pos


def shuffled_list(n, seed, count=None):
    """Pairs in any order with duplicates; the first and the last pair of the triangle are in it."""
    from eagleeverything_amd import r_api
    allp = r_api.ibd_all_pairs(n)
    rng = np.random.default_rng(seed)
    k = np.concatenate(([allp.shape[0] - 1, 0, allp.shape[0] - 1], rng.integers(0, allp.shape[0], count or min(3 * allp.shape[0] // 2, 700))))
    return allp[k], k


def rows_of_list(tab_all, seg_all, k):
    """What a list of the pair ordinals k must return, from the all-pairs tables."""
    offs = np.concatenate(([0], np.cumsum(tab_all[:, 0])))
    seg = [seg_all[offs[o]:offs[o + 1]] for o in k.tolist()]
    return tab_all[k], np.concatenate(seg).reshape(-1, 6) if seg else np.zeros((0, 6), dtype=np.int32)


@pytest.mark.parametrize("n", NS)
def test_gpu_ibd_equals_host_at_word_edges(tmp_path, n):
    from eagleeverything_amd import r_api, rcpp_api
    rcpp_api.drop_cache()
    some = merged = 0
    for L in LS:
        g, _ = T.mosaic(n, L, 2, seed=1000 * n + L, noise=0.03)
        g[L - 1, 0], g[L - 1, n - 1] = -1, 1             # a break on the last marker of the panel for the pair (0, n - 1)
        M = write_M(tmp_path, g, "M%d.ascii" % L)
        for mode in (1, 2):
            for merge_min in (0, 2):
                prm = dict(mode=mode, min_snp=1 if L < 3 else 2, merge_min=merge_min)
                want = r_api.ibd_host(g, **prm)
                same(rcpp_api.ibd(M, (n, L), **prm), want, (n, L, prm))
                assert np.all(want[1][:, 5] == 0)
                some += want[1].shape[0]
                merged += int((want[1][:, 4] > 0).sum())
    assert some > 0 and merged > 0
    rcpp_api.drop_cache()


@pytest.mark.parametrize("v", range(len(VARIANTS)))
@pytest.mark.parametrize("n", NS)
def test_gpu_ibd_mosaic_panel_all_pairs_and_a_list(tmp_path, n, v):
    from eagleeverything_amd import r_api, rcpp_api
    g, _, chrom, pos = mosaic_panel(n)
    M = write_M(tmp_path, g)
    rcpp_api.drop_cache()
    prm = VARIANTS[v]
    for mode in (1, 2):
        want = r_api.ibd_host(g, None, None, chrom, pos, mode=mode, **prm)
        got = rcpp_api.ibd(M, (n, LM), None, chrom, pos, mode=mode, **prm)
        same(got, want, (n, v, mode, "all pairs"))
        assert want[1].shape[0] >= 1 and (prm["merge_min"] == 0 or (want[1][:, 4] >= 1).any())
        planted = want[1][(want[1][:, 0] == n - 2) & (want[1][:, 1] == n - 1)]
        assert planted.shape[0] >= 3 and set(planted[:, 5].tolist()) == {0, 1, 2, 3}
        pairs, k = shuffled_list(n, seed=7 * n + v)
        lst = rcpp_api.ibd(M, (n, LM), pairs, chrom, pos, mode=mode, **prm)
        same(lst, rows_of_list(got[0], got[1], k), (n, v, mode, "a list against all pairs, pair by pair"))
    rcpp_api.drop_cache()


def test_gpu_ibd_planted_cases(tmp_path):
    """Pair (0, 1) is two copies of one individual with breaks at the planted markers: the tables are known without a reference."""
    from eagleeverything_amd import rcpp_api
    n = 3
    g, _, chrom, _ = mosaic_panel(n)
    M = write_M(tmp_path, g)
    rcpp_api.drop_cache()
    s0 = SEQ_AT + 1
    for mode in (1, 2):
        def seq(**prm):
            _, seg = rcpp_api.ibd(M, (n, LM), [[0, 1]], chrom, None, mode=mode, **prm)
            return [r[2:5] for r in seg.tolist() if SEQ_AT <= r[2] and r[3] < SEQ_AT + 170]
        # no merging: the runs of at least min_snp markers, each on its own
        assert seq(min_snp=30, merge_min=0) == [[s0, s0 + 29, 0]]
        assert seq(min_snp=20, merge_min=0) == [[s0, s0 + 29, 0], [s0 + 31, s0 + 59, 0], [s0 + 82, s0 + 101, 0]]
        # merge_min = 10: 30 | 29 | 10 chain up, the run of 9 is on its own and keeps 20 | 19 apart from them; 3 and 2 are too short
        assert seq(min_snp=20, merge_min=10) == [[s0, s0 + 70, 2], [s0 + 82, s0 + 121, 1]]
        # merge_min = 1: the whole block [1280, 1921) between its first and last breaks is two chains, apart at the two breaks in a row
        end = s0 + sum(SEQ_RUNS) + len(SEQ_RUNS) - 2
        _, seg = rcpp_api.ibd(M, (n, LM), [[0, 1]], chrom, None, mode=mode, min_snp=12, merge_min=1)
        assert [r[2:5] for r in seg.tolist() if r[5] == 2] == [[1281, end, len(SEQ_RUNS) + 1], [end + 3, 1918, 3]]
    rcpp_api.drop_cache()


def test_gpu_ibd_capacity(tmp_path):
    """seg_cap = 0 returns the totals, seg_cap = total fills the rows, seg_cap = total - 1 leaves the buffer untouched."""
    from eagleeverything_amd import _lib, r_api, rcpp_api
    n = 65
    g, _, chrom, pos = mosaic_panel(n)
    M = write_M(tmp_path, g)
    rcpp_api.drop_cache()
    kw = dict(mode=1, min_snp=30, merge_min=10)
    want_tab, want_seg = r_api.ibd_host(g, None, None, chrom, pos, **kw)
    total, P = want_seg.shape[0], n * (n - 1) // 2
    assert total > 10
    lib, ctx = _lib.load(), rcpp_api.context(0)
    p = dict(rcpp_api.IBD_DEFAULTS, **kw)
    prm = _lib.IbdParams(*[p[f] for f in rcpp_api._IBD_FIELDS])
    dims = (C.c_long * 2)(n, LM)
    ch, ps = np.ascontiguousarray(chrom), np.ascontiguousarray(pos)

    def call(seg, cap):
        tab, got = np.zeros((P, 4), dtype=np.int64), C.c_long(-1)
        rc = lib.eagle_ibd(ctx, os.fsencode(M), dims, None, 0, ch.ctypes.data_as(C.POINTER(C.c_int32)), ps.ctypes.data_as(C.POINTER(C.c_int64)),
                           C.addressof(prm), 8.0, tab.ctypes.data_as(C.POINTER(C.c_int64)),
                           seg.ctypes.data_as(C.POINTER(C.c_int32)) if seg is not None else None, cap, C.byref(got))
        assert rc == 0
        return tab, got.value
    tab, got = call(None, 0)
    assert got == total and np.array_equal(tab, want_tab)
    seg = np.full((total + 1, 6), -7, dtype=np.int32)
    tab, got = call(seg, total)
    assert got == total and np.array_equal(tab, want_tab) and np.array_equal(seg[:total], want_seg) and np.all(seg[total] == -7)
    seg = np.full((total, 6), -7, dtype=np.int32)
    tab, got = call(seg, total - 1)
    assert got == total and np.array_equal(tab, want_tab) and np.all(seg == -7)
    tab, seg = rcpp_api.ibd(M, (n, LM), None, chrom, pos, seg_cap=1, **kw)               # the wrapper calls once more
    assert np.array_equal(tab, want_tab) and np.array_equal(seg, want_seg)
    rcpp_api.drop_cache()


def test_gpu_ibd_streamed_equals_resident(tmp_path, monkeypatch):
    """700 individuals x 2,100 markers is 1.8 MB of image: under a budget of 1 MB it goes in three bands of whole lines."""
    from eagleeverything_amd import r_api, rcpp_api
    n = 700
    g, _ = T.mosaic(n, LM, 4, seed=77)
    chrom, pos = chrom_of(list(LENGTHS)), pos_of(list(LENGTHS), seed=3)
    rng = np.random.default_rng(8)
    i = np.concatenate((rng.integers(0, n - 1, 1500), [0, 255, 255, 256, 511, 511, 0, 698]))      # pairs inside and across the bands
    j = np.concatenate((rng.integers(1, n, 1500), [255, 256, 699, 511, 512, 699, 699, 699]))
    keep = i != j
    pairs = np.stack([np.minimum(i, j)[keep], np.maximum(i, j)[keep]], axis=1)
    M = write_M(tmp_path, g)
    cases = [dict(mode=1, **VARIANTS[1]), dict(mode=2, **VARIANTS[2])]
    rcpp_api.drop_cache()
    resident = []
    for prm in cases:
        want = r_api.ibd_host(g, None, pairs, chrom, pos, **prm)
        resident.append(rcpp_api.ibd(M, (n, LM), pairs, chrom, pos, **prm))
        same(resident[-1], want, ("resident", prm["mode"]))
        assert want[1].shape[0] >= 16 and (want[1][:, 4] >= 1).any()
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.001")
    for prm, res in zip(cases, resident):
        same(rcpp_api.ibd(M, (n, LM), pairs, chrom, pos, **prm), res, ("streamed", prm["mode"]))
    rcpp_api.drop_cache()


def test_gpu_ibd_view_alias_gives_the_kept_individuals(tmp_path):
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    n, L = 70, 300
    g, _ = T.mosaic(n, L, 3, seed=12)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), g)
    drop = np.array([1, 2, 33, 64, 65, 70])              # 1-based, as AM's indxNA
    kept = np.setdiff1d(np.arange(n), drop - 1)
    sub = am.reshape_geno(geno, drop, view=True)
    nk = n - drop.size
    assert list(sub["dim_of_ascii_M"]) == [nk, L]
    own = str(tmp_path / "own.ascii")
    synth.write_ascii(own, np.ascontiguousarray(g[:, kept].T))
    prm = dict(mode=2, min_snp=20, merge_min=5)
    got = rcpp_api.ibd(sub["asciifileM"], (nk, L), **prm)
    same(got, rcpp_api.ibd(own, (nk, L), **prm), "view against the subset's own file")
    same(got, r_api.ibd_host(g[:, kept], **prm), "view against the host")
    assert got[1].shape[0] > 0
    rcpp_api.drop_cache()
