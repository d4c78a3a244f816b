"""LD scores and the LD decay curve on the GPU: eagle_ld_stats (k_ld_tile's r2 mode on the int8 MFMA, k_ld_reduce) and LDScore / LDDecay /
GRM(ld_score=) on top.

The device's sums are compared with r_api.ld_stats_host(r_api.ld_band_host(...)) -- the numpy restatement that
tests/test_ld_stats_host.py pins to plain loops of the definitions (include/eagle_hip.h section 1b'''v).  U, cnt, bin_sum and bin_pairs
are integers: every comparison is ==."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WINDOWS = (1, 33, 50, 256)


def partner_panel(n, L, seed):
    """Random genotypes with what the shapes allow: identical markers across the 128-marker tile edge and the 32-row block edge (ties in
    r2, seen from one side and from both), monomorphic markers beside those edges."""
    from eagleeverything_amd import synth
    Mt8 = synth.genotypes_marker_major(n, L, seed=seed)
    if L >= 129:
        Mt8[127] = Mt8[128] = Mt8[124]
        Mt8[126] = 1
        Mt8[31] = Mt8[33] = Mt8[32]
        Mt8[30] = 0
    if L >= 300:
        Mt8[255] = Mt8[256] = Mt8[258]
        Mt8[257] = -1
        Mt8[299] = Mt8[297]
    return Mt8


def chrom_of(L):
    return (3 - (np.arange(L) >= 70) - (np.arange(L) >= 200)).astype(np.int32)      # 3, 2, 1: changes inside the tiles, not sorted


def pos_of(L):
    """Base pairs, 1,000 apart, every seventh marker 2,500 further on: not monotone."""
    return (np.arange(L, dtype=np.int64) * 1000 + np.where(np.arange(L) % 7 == 3, 2500, 0)).astype(np.int64)


MAX_DIST = 20000                                         # about 20 markers: cuts inside the windows 33, 50 and 256
COARSE = [2, 4, 9, 30]                                   # three bins of offsets: offset 1 and offsets from 30 on are in no bin
COARSE_BP = [1500, 3000, 9000, 15000]                    # three bins of base pairs, pairs left out at both ends


def variants(L, window):
    return (dict(),
            dict(chrom=chrom_of(L)),
            dict(pos=pos_of(L), max_dist=MAX_DIST),
            dict(edges=np.arange(1, window + 2)),                                               # one bin per offset
            dict(chrom=chrom_of(L), edges=COARSE),
            dict(chrom=chrom_of(L), pos=pos_of(L), max_dist=MAX_DIST, edges=COARSE_BP),
            dict(pos=pos_of(L), edges=np.arange(513) * 45))                                     # B = 512, pos without max_dist


def same(got, want, what):
    assert len(got) == len(want), what
    for g, w, dt in zip(got, want, (np.uint64, np.int32, np.uint64, np.int64)):
        assert g.dtype == dt and g.shape == w.shape, what
        assert np.array_equal(g, w), (what, np.flatnonzero(g != w)[:10])


@pytest.mark.parametrize("n", [1, 3, 65, 257])
@pytest.mark.parametrize("L", [1, 2, 129, 300])
def test_gpu_ld_stats_equals_host(tmp_path, n, L):
    from eagleeverything_amd import r_api, rcpp_api, synth
    Mt8 = partner_panel(n, L, seed=1000 * n + L)
    Mt = str(tmp_path / "Mt.ascii")
    synth.write_ascii(Mt, Mt8)
    rcpp_api.drop_cache()
    for window in WINDOWS:
        band = r_api.ld_band_host(Mt8, window)
        for kw in variants(L, window):
            want = r_api.ld_stats_host(band, **kw)
            got = rcpp_api.ld_stats(Mt, (n, L), window, **kw)
            same(got, want, (n, L, window, sorted(kw)))
            if n == 1:                                                        # every marker is monomorphic
                assert all(not g.any() for g in got)
    if L >= 129 and n >= 65:
        U, cnt, bsum, bpairs = rcpp_api.ld_stats(Mt, (n, L), 50, edges=[1, 2, 51])
        assert U[126] == 0 and cnt[126] == 0 and U[30] == 0 and cnt[30] == 0                    # monomorphic: score 1.0
        assert U[127] >= 2 << 30 and U[32] >= 2 << 30                                           # two identical markers each
        assert int(U.sum(dtype=np.uint64)) == 2 * int(bsum.sum(dtype=np.uint64)) and int(cnt.sum()) == 2 * int(bpairs.sum())
    rcpp_api.drop_cache()


def test_gpu_ld_stats_more_marker_groups_than_workgroups(tmp_path):
    """More than 4 x 2,048 markers in one core: the workgroups walk the marker groups with the grid's stride and flush once."""
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L = 3, 8500
    Mt8 = synth.genotypes_marker_major(n, L, seed=5)
    Mt = str(tmp_path / "Mt.ascii")
    synth.write_ascii(Mt, Mt8)
    rcpp_api.drop_cache()
    for window, kw in ((5, dict(edges=np.arange(1, 7))), (33, dict(pos=pos_of(L), max_dist=MAX_DIST, edges=COARSE_BP))):
        same(rcpp_api.ld_stats(Mt, (n, L), window, **kw), r_api.ld_stats_host(r_api.ld_band_host(Mt8, window), **kw), (window,))
    rcpp_api.drop_cache()


@pytest.fixture(scope="module")
def streamed_panel():
    """n = 65, L = 5,000 with strong pairs around the rows where row windows of 1,792 and 2,048 rows end; the host's sums, once."""
    from eagleeverything_amd import r_api, synth
    n, L = 65, 5000
    Mt8 = synth.genotypes_marker_major(n, L, seed=77)
    for a in (1500, 1791, 1792, 2047, 2048, 3400):
        Mt8[a + 1], Mt8[a - 40], Mt8[a + 200] = Mt8[a], -Mt8[a], Mt8[a]
    Mt8[1793], Mt8[2049] = 0, 1
    chrom = (np.arange(L) >= 1800).astype(np.int32)
    pos = pos_of(L)
    cases = {}
    for window in (50, 256):
        band = r_api.ld_band_host(Mt8, window)
        for name, kw in (("offsets", dict(edges=np.arange(1, window + 2))),
                         ("map", dict(chrom=chrom, pos=pos, max_dist=40000, edges=np.arange(0, 40001, 800)))):     # d = 40,000: in no bin
            cases[(window, name)] = (kw, r_api.ld_stats_host(band, **kw))
    Mt8.setflags(write=False)
    return n, L, Mt8, chrom, pos, cases


def test_gpu_ld_stats_streamed_equals_resident(tmp_path, monkeypatch, streamed_panel):
    from eagleeverything_amd import rcpp_api, synth
    n, L, Mt8, chrom, pos, cases = streamed_panel
    path = str(tmp_path / "Mt.ascii")
    synth.write_ascii(path, Mt8)
    rcpp_api.drop_cache()
    resident = {}
    for (window, name), (kw, want) in cases.items():
        resident[(window, name)] = rcpp_api.ld_stats(path, (n, L), window, **kw)
        same(resident[(window, name)], want, (window, name, "resident"))
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.001")                  # 1 MB: the 5,120 x 256 image goes in at least 3 row windows
    for (window, name), (kw, want) in cases.items():
        got = rcpp_api.ld_stats(path, (n, L), window, **kw)
        same(got, want, (window, name, "streamed"))                           # a pair counted in two cores, or in none, shows here
        same(got, resident[(window, name)], (window, name, "streamed against resident"))
    rcpp_api.drop_cache()


def test_gpu_ldscore_lddecay_and_the_weighted_grm(tmp_path, streamed_panel):
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L, Mt8, chrom, pos, cases = streamed_panel
    bed = synth.write_bed(str(tmp_path / "panel"), Mt8)
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(tmp_path))
    assert list(geno["dim_of_ascii_M"]) == [n, L]
    map = {"SNP": ["m%d" % i for i in range(L)], "Chr": ["chrB" if c else "chrA" for c in chrom], "Pos": [int(p) for p in pos]}
    band = r_api.ld_band_host(Mt8, 50)
    # scores
    res = r_api.LDScore(geno)
    U, cnt = r_api.ld_stats_host(band)
    assert np.array_equal(res["u"], U) and np.array_equal(res["partners"], cnt) and res["score"].dtype == np.float64
    assert np.array_equal(res["score"], 1.0 + U.astype(np.float64) * 2.0 ** -30) and res["score"][1793] == 1.0 and res["score"].min() >= 1.0
    res_map = r_api.LDScore(geno, map=map, kb=40)
    U, cnt = r_api.ld_stats_host(band, chrom=chrom, pos=pos, max_dist=40000)
    assert np.array_equal(res_map["u"], U) and np.array_equal(res_map["partners"], cnt) and cnt.max() < 100
    with pytest.raises(ValueError):
        r_api.LDScore(geno, kb=40)                                            # kb needs a map
    # decay: the defaults without a map are one bin per offset
    kw, (U, cnt, bsum, bpairs) = cases[(256, "offsets")]
    dec = r_api.LDDecay(geno)
    mean = bsum.astype(np.float64) / bpairs.astype(np.float64) * 2.0 ** -30
    assert np.array_equal(dec["edges"], np.arange(1, 258)) and np.array_equal(dec["pairs"], bpairs) and np.array_equal(dec["sum"], bsum)
    assert np.array_equal(dec["mean_r2"], mean) and dec["half_decay"] == r_api.ld_half_decay(dec["edges"], bpairs, mean)
    # ... and with a map 50 equal bins up to kb
    kw, (U, cnt, bsum, bpairs) = cases[(256, "map")]
    assert kw["edges"].size == 51 and kw["edges"][-1] == 40000
    edges = np.unique(np.rint(np.linspace(0.0, 40001.0, 51)).astype(np.int64))
    want = r_api.ld_stats_host(r_api.ld_band_host(Mt8, 256), chrom=chrom, pos=pos, max_dist=40000, edges=edges)
    dec = r_api.LDDecay(geno, map=map, kb=40)
    assert np.array_equal(dec["edges"], edges) and edges.size == 51
    assert np.array_equal(dec["pairs"], want[3]) and np.array_equal(dec["sum"], want[2]) and int(want[3].sum()) > L
    dec = r_api.LDDecay(geno, map=map, kb=40, bins=kw["edges"])               # the caller's own edges
    assert np.array_equal(dec["pairs"], bpairs) and np.array_equal(dec["sum"], bsum)
    with pytest.raises(ValueError):
        r_api.LDDecay(geno, map=map)                                          # a map needs kb
    # the relationship matrix with every marker's weight divided by its LD score
    score = res["score"]
    stats = r_api.MarkerStats(geno)
    for method in ("standardized", "vanraden1"):
        grm = r_api.GRM(geno, method=method, stats=stats, ld_score=score)
        q, scale, used = r_api.grm_weights(stats["n0"], stats["n1"], stats["n2"], method=method, ld_score=score)
        assert np.array_equal(grm["q"], q) and grm["scale"] == scale and np.array_equal(grm["used"], used)
        Q = rcpp_api.weighted_gram(geno["asciifileM"], (n, L), q)
        info = {"method": method, "scale": scale, "used": used, "q": q, "n0": stats["n0"], "n1": stats["n1"], "n2": stats["n2"]}
        assert np.array_equal(grm["Q"], Q) and np.array_equal(grm["G"], r_api.grm_from_gram(Q, info))
        assert not np.array_equal(grm["q"], r_api.grm_weights(stats["n0"], stats["n1"], stats["n2"], method=method)[0])
    rcpp_api.drop_cache()
