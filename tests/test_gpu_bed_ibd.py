"""Pairwise IBD-type segments on the GPU from the .bed file: eagle_bed_ibd (k_ibd_planes_bed, k_ibd_walk), which still knows the missing
calls -- a marker where either individual is not called is never a break -- and r_api.IBD on top of both routes.

The device's tables are compared with r_api.ibd_host(*r_api.ibd_genotypes_bed(read_bed_codes(...))) -- the numpy restatement that
tests/test_ibd_host.py pins to plain loops of the definitions (include/eagle_hip.h section 1b'''vii) -- and, on a file without a missing
code, with rcpp_api.ibd of the ingested panel.  Everything is integers: every comparison is ==."""
import os

import numpy as np
import pytest

import ibd_truth as T
from conftest import GOLDEN
from test_gpu_bed_ld_stats import write_bed              # pad bit pairs of a row's last byte set to 01 and 11
from test_gpu_ibd import LM, LS, NS, VARIANTS, mosaic_panel, planted_markers, rows_of_list, same, shuffled_list

pytestmark = pytest.mark.gpu

PREFIX = os.path.join(GOLDEN, "plink_150x100")
SMALL_GB = 1e-4                                          # staging windows of 25,000 bytes: 757 rows at n = 129


def panel_of(tmp_path, name, g, called, include=None, seed=0):
    """Writes the fileset of the panel (g, called); with include = a file length, the panel's markers are a selection of that many file
    markers (the others are noise) -> (bed, file markers, include mask or None)."""
    L, n = g.shape
    if include is None:
        return write_bed(tmp_path, name, g, ~called), L, None
    rng = np.random.default_rng(seed)
    inc = np.zeros(include, dtype=bool)
    free = np.setdiff1d(np.arange(include), [0, 63, 64, 127, 128, 129, include - 1])    # markers dropped at word edges of the file
    inc[rng.choice(free, L, replace=False)] = True
    gf = rng.integers(-1, 2, (include, n)).astype(np.int8)
    cf = np.ones((include, n), dtype=bool)
    gf[inc], cf[inc] = g, called
    return write_bed(tmp_path, name, gf, ~cf), include, inc


@pytest.mark.parametrize("n", NS)
def test_gpu_bed_ibd_equals_host_at_word_edges(tmp_path, n):
    from eagleeverything_amd import r_api, rcpp_api
    some = hidden = 0
    for L in LS:
        g, called = T.mosaic(n, L, 2, seed=2000 * n + L, noise=0.03, miss=0.05)
        bed = write_bed(tmp_path, "p%d" % L, g, ~called)
        codes = r_api.read_bed_codes(bed, (n, L))
        gg, cc = r_api.ibd_genotypes_bed(codes)
        assert np.array_equal(cc, called) and np.array_equal(gg, g)
        for mode in (1, 2):
            prm = dict(mode=mode, min_snp=1 if L < 3 else 2, merge_min=(0, 2)[mode - 1])
            want = r_api.ibd_host(gg, cc, **prm)
            same(rcpp_api.bed_ibd(bed, (n, L), **prm), want, (n, L, prm))
            some += want[1].shape[0]
            hidden += int(want[0][:, 1].sum() - r_api.ibd_host(gg, None, **prm)[0][:, 1].sum() != 0)
    assert some > 0 and hidden > 0                       # the missing calls matter: as hets they give other tables
    rcpp_api.drop_cache()


@pytest.mark.parametrize("v", range(len(VARIANTS)))
@pytest.mark.parametrize("n", NS)
def test_gpu_bed_ibd_mosaic_panel_with_missing_calls_and_include(tmp_path, n, v):
    """miss = 0.05, n not a multiple of 4 among the shapes, the panel a selection of the file's markers (which moves every word edge of
    the panel off the file's), small staging windows for two of the variants."""
    from eagleeverything_amd import r_api, rcpp_api
    g, called, chrom, pos = mosaic_panel(n, 0.05)
    Lf = LM + LM // 6 if v else LM
    bed, Lf, inc = panel_of(tmp_path, "m", g, called, Lf if v else None, seed=n)
    codes = r_api.read_bed_codes(bed, (n, Lf))
    gg, cc = r_api.ibd_genotypes_bed(codes if inc is None else codes[inc])
    assert np.array_equal(cc, called) and np.array_equal(gg, g)
    mem = SMALL_GB if v != 1 else 8.0
    prm = VARIANTS[v]
    hid = planted_markers()[1]
    for mode in (1, 2):
        want = r_api.ibd_host(gg, cc, None, chrom, pos, mode=mode, **prm)
        got = rcpp_api.bed_ibd(bed, (n, Lf), inc, None, chrom, pos, mem, mode=mode, **prm)
        same(got, want, (n, v, mode, "all pairs"))
        assert want[1].shape[0] >= 1 and (prm["merge_min"] == 0 or (want[1][:, 4] >= 1).any())
        mine = want[1][(want[1][:, 0] == n - 2) & (want[1][:, 1] == n - 1)]
        assert any(r[2] <= hid <= r[3] and (r[4] == 0 or prm["merge_min"]) for r in mine.tolist())     # no break at the hidden marker
        pairs, k = shuffled_list(n, seed=11 * n + v)
        lst = rcpp_api.bed_ibd(bed, (n, Lf), inc, pairs, chrom, pos, mem, mode=mode, **prm)
        same(lst, rows_of_list(got[0], got[1], k), (n, v, mode, "a list against all pairs, pair by pair"))
    rcpp_api.drop_cache()


def test_gpu_bed_ibd_capacity_and_window_size(tmp_path):
    """seg_cap one below the total leaves the rows out and returns the total; the tables do not depend on the staging window."""
    from eagleeverything_amd import r_api, rcpp_api
    n = 65
    g, called, chrom, pos = mosaic_panel(n, 0.05)
    bed = write_bed(tmp_path, "c", g, ~called)
    kw = dict(mode=2, min_snp=30, merge_min=10)
    want = r_api.ibd_host(g, called, None, chrom, pos, **kw)
    total = want[1].shape[0]
    assert total > 10
    for mem in (8.0, SMALL_GB, 2e-5):
        same(rcpp_api.bed_ibd(bed, (n, LM), None, None, chrom, pos, mem, seg_cap=total, **kw), want, mem)
        same(rcpp_api.bed_ibd(bed, (n, LM), None, None, chrom, pos, mem, seg_cap=total - 1, **kw), want, (mem, "grown"))
    rcpp_api.drop_cache()


def test_gpu_bed_ibd_without_missing_is_the_ingested_panel(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    n = 129
    g, called, chrom, pos = mosaic_panel(n)
    bed = write_bed(tmp_path, "full", g, ~called)
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(tmp_path))
    assert list(geno["dim_of_ascii_M"]) == [n, LM]
    for v, prm in enumerate(VARIANTS):
        mode = 1 + v % 2
        a = rcpp_api.bed_ibd(bed, (n, LM), None, None, chrom, pos, SMALL_GB, mode=mode, **prm)
        b = rcpp_api.ibd(geno["asciifileM"], (n, LM), None, chrom, pos, mode=mode, **prm)
        same(a, b, "bed against the ingested panel")
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[1].shape[0] > 0
    rcpp_api.drop_cache()


def test_gpu_IBD_end_to_end_on_the_golden_fileset(tmp_path):
    """r_api.IBD on tests/golden/plink_150x100 (4 chromosomes of 25 markers, 10 kb apart) with small thresholds, both routes, with and
    without a map, all pairs and Relatedness' list; ibd_kinship on top."""
    from eagleeverything_amd import r_api, rcpp_api
    n, L = 150, 100
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(PREFIX, type="PLINKbed", outdir=str(tmp_path))
    g, called = r_api.ibd_genotypes_bed(r_api.read_bed_codes(PREFIX, (n, L)))
    map = r_api.ReadBim(PREFIX + ".bim")
    chrom, pos = np.repeat(np.arange(4), 25).astype(np.int32), np.asarray(map["Pos"], dtype=np.int64)
    assert [str(c) for c in map["Chr"]] == [str(c + 1) for c in chrom.tolist()] and np.all(np.diff(pos) == 10000)
    out = {}
    for mode in ("ibs1", "ibs2"):
        # without a map: one block, lengths in markers, the kb arguments must be None
        res = r_api.IBD(geno, mode=mode, min_snp=5, merge_min_snp=2, min_kb=None, max_gap_kb=None)
        tab, seg = r_api.ibd_host(g, None, mode=mode, min_snp=5, merge_min=2)
        assert np.array_equal(res["pair"], tab) and np.array_equal(res["seg"], seg) and seg.shape[0] > 0
        assert np.array_equal(res["shared"], tab[:, 2] / np.float64(L - 1)) and np.array_equal(res["ibd_incidence"], r_api.ibd_incidence(seg, L))
        assert np.array_equal(res["pairs"], r_api.ibd_all_pairs(n))
        with pytest.raises(ValueError):
            r_api.IBD(geno, mode=mode)
        # with a map, from the panel and from the file (no missing code in it: the same tables)
        want = r_api.ibd_host(g, called, None, chrom, pos, mode=mode, min_snp=5, merge_min=2, min_len=50000, max_gap=10000)
        ref = r_api.ibd_summary(r_api.ibd_all_pairs(n), want[0], want[1], L, chrom, pos)
        for bed in (None, PREFIX):
            res = r_api.IBD(geno, map=map, bed=bed, mode=mode, min_snp=5, merge_min_snp=2, min_kb=50, max_gap_kb=10)
            assert np.array_equal(res["pair"], want[0]) and np.array_equal(res["seg"], want[1]) and want[1].shape[0] > 0
            assert np.array_equal(res["shared"], want[0][:, 2] / np.float64(4 * 24 * 10000))
            for k in ref["segments"]:
                assert np.array_equal(res["segments"][k], ref["segments"][k]), k
        assert r_api.IBD(geno, map=map, mode=mode, min_snp=5, merge_min_snp=2, min_kb=50, max_gap_kb=9.999)["seg"].shape[0] == 0   # every step is a cut
        out[mode] = res
    kin = r_api.ibd_kinship(out["ibs1"], out["ibs2"])
    assert kin.shape == (n * (n - 1) // 2,) and np.all((kin >= 0) & (kin <= 0.5)) and kin.max() > 0
    # the pairs Relatedness reports
    rel = r_api.Relatedness(geno, threshold=0.0)["pairs"]
    assert rel.shape[0] > 0
    res = r_api.IBD(geno, map=map, pairs=rel, mode="ibs1", min_snp=5, merge_min_snp=2, min_kb=50, max_gap_kb=10)
    want = r_api.ibd_host(g, None, rel, chrom, pos, mode=1, min_snp=5, merge_min=2, min_len=50000, max_gap=10000)
    assert np.array_equal(res["pair"], want[0]) and np.array_equal(res["seg"], want[1]) and np.array_equal(res["pairs"], rel)
    rcpp_api.drop_cache()
