"""Pairwise haplotype EM on the GPU: eagle_hap_ld (k_hapld_tile on the int8 MFMA with its fp64 epilogue; include/eagle_hip.h section
1b''''vii) and HapLD / HapBlocks / sets_from_blocks on top.  Expected values are r_api.hap_ld_host's -- which tests/test_hapld_host.py
holds to counting loops, a scalar loop of the rule and mpmath -- and every comparison is exact: masks, both fp64 bands and counts."""
import numpy as np
import pytest

import hapld_truth as T

pytestmark = pytest.mark.gpu

WINDOWS = (1, 33, 50, 256)      # NB = 2, 3, 3, 9 block offsets: one group of 2, one of 3, three groups of 3


def same(got, want, what):
    for key, dt in (("recomb", np.uint64), ("strong", np.uint64), ("dprime", np.float64), ("r2", np.float64), ("counts", np.int64)):
        if key not in got:
            continue
        g, w = got[key], want[key]
        assert g.dtype == dt and g.shape == w.shape, (what, key)
        assert np.array_equal(g, w), (what, key, np.argwhere(g != w)[:10].tolist())


@pytest.mark.parametrize("n", [1, 3, 65, 257])
@pytest.mark.parametrize("L", [1, 2, 129, 300])
def test_gpu_hap_ld_equals_host(tmp_path, n, L):
    from eagleeverything_amd import r_api, rcpp_api, synth
    Mt8 = T.partner_panel(n, L, seed=1000 * n + L)
    Mt = str(tmp_path / "Mt.ascii")
    synth.write_ascii(Mt, Mt8)
    rcpp_api.drop_cache()
    for window in WINDOWS:
        want = r_api.hap_ld_host(Mt8, window)
        got = rcpp_api.hap_ld(Mt, (n, L), window, bands=True)
        same(got, want, (n, L, window))
        if n == 1:                                                            # nothing is defined
            assert not got["counts"].any() and not got["recomb"].any() and (got["dprime"] == -2.0).all() and (got["r2"] == -1.0).all()
    only = rcpp_api.hap_ld(Mt, (n, L), 50)                                    # masks alone
    assert sorted(only) == ["counts", "recomb", "strong"]
    same(only, r_api.hap_ld_host(Mt8, 50), (n, L, "masks only"))
    want = r_api.hap_ld_host(Mt8, 50, max_iter=3, fg_cut=0.05, dprime_cut=0.5)
    got = rcpp_api.hap_ld(Mt, (n, L), 50, max_iter=3, fg_cut=0.05, dprime_cut=0.5, bands=True, masks=False)
    same(got, want, (n, L, "max_iter 3"))
    assert sorted(got) == ["counts", "dprime", "r2"]
    if L >= 129 and n >= 65:
        assert got["counts"][1] > 0 and got["counts"][1] == int((want["code"] == 1).sum())      # pairs forced to stop with code 1
        full = rcpp_api.hap_ld(Mt, (n, L), 50, bands=True)
        assert T.bit(full["strong"], 124, 127) and T.bit(full["strong"], 127, 128) and full["dprime"][127, 0] == -1.0      # across the tile edge
        assert T.bit(full["strong"], 31, 32) and full["dprime"][32, 0] == -1.0 and full["dprime"][31, 1] == -1.0          # across the block edge
        assert not T.bit(full["recomb"], 31, 32) and not T.bit(full["recomb"], 127, 128)
        for m in (30, 126):                                                                       # monomorphic: undefined from both sides
            assert (full["dprime"][m] == -2.0).all() and all(full["dprime"][m - o, o - 1] == -2.0 for o in range(1, 20))
    rcpp_api.drop_cache()


@pytest.fixture(scope="module")
def streamed_panel():
    """n = 65, L = 5,000 with strong and recombinant pairs planted around the rows where row windows of 1,792 and 2,048 rows end; the
    host's words, once."""
    from eagleeverything_amd import r_api, synth
    n, L = 65, 5000
    Mt8 = synth.genotypes_marker_major(n, L, seed=78)
    rng = np.random.default_rng(78)
    for a in (1500, 1791, 1792, 2047, 2048, 3400):
        Mt8[a + 1], Mt8[a - 40], Mt8[a + 200] = Mt8[a], -Mt8[a], Mt8[a]      # strong: identical and negated
        hap = rng.random((2, 2 * n)) < 0.5                                    # recombinant: independent haplotypes at 0.5
        Mt8[a - 3], Mt8[a + 3] = (hap[:, 0::2].astype(np.int8) + hap[:, 1::2] - 1).astype(np.int8)
    Mt8[1793], Mt8[2049] = -1, 1                                              # monomorphic
    Mt8.setflags(write=False)
    return n, L, Mt8, r_api.hap_ld_host(Mt8, 50)


def ingest(tmp, name, Mt8):
    from eagleeverything_amd import r_api, synth
    d = tmp / name
    d.mkdir()
    bed = synth.write_bed(str(d / "panel"), Mt8)
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(d))
    assert list(geno["dim_of_ascii_M"]) == [Mt8.shape[1], Mt8.shape[0]]
    return geno


def test_gpu_hap_ld_streamed_routes_equal_resident(tmp_path, monkeypatch, streamed_panel):
    from eagleeverything_amd import r_api, rcpp_api
    n, L, Mt8, want = streamed_panel
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, "p", Mt8)
    Mt = geno["asciifileMt"]
    resident = {w: rcpp_api.hap_ld(Mt, (n, L), w, bands=True) for w in (50, 256)}
    same(resident[50], want, "resident")
    wide = resident[256]
    assert wide["counts"][0] > 4 * want["counts"][0] and np.array_equal(wide["dprime"][:, :50], want["dprime"])
    for a in (1791, 1792, 2047, 2048):
        assert T.bit(wide["strong"], a - 40, a) and T.bit(wide["strong"], a, a + 200) and T.bit(wide["recomb"], a - 3, a + 3)
        assert T.bit(wide["strong"], a, a + 1) == (a in (1791, 2047)) and (wide["dprime"][a, 0] == -2.0) == (a in (1792, 2048))
    # a VIEW alias, resident: five individuals fewer
    na = np.array([1, 2, 30, 64, 65])                                         # 1-based, as R hands them over
    kept = np.setdiff1d(np.arange(n), na - 1)
    dims = r_api.ReshapeM(geno["asciifileM"], Mt, na, (n, L), view=True)
    assert dims[0] == n - 5
    sub = np.ascontiguousarray(Mt8[:, kept])
    want_view = r_api.hap_ld_host(sub, 50)
    assert not np.array_equal(want_view["strong"], resident[50]["strong"])   # the five individuals matter
    same(rcpp_api.hap_ld(Mt + "tmp", (n - 5, L), 50, bands=True), want_view, "view, resident")
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.001")                  # 1 MB: the 5,120 x 256 image goes in row windows of 2,048 rows
    for sidecar in ("1", "0"):                                                # from the sidecar, then from the text
        monkeypatch.setenv("EAGLE_HIP_SIDECAR", sidecar)
        for w in (50, 256):
            same(rcpp_api.hap_ld(Mt, (n, L), w, bands=True), resident[w], ("streamed", sidecar, w))
        same(rcpp_api.hap_ld(Mt + "tmp", (n - 5, L), 50, bands=True), want_view, ("view, streamed", sidecar))
    rcpp_api.drop_cache()


def test_gpu_hapblocks_hapld_and_settest(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    Mt8, bounds = T.planted_blocks()
    L, n = Mt8.shape
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, "p", Mt8)
    host = r_api.hap_ld_host(Mt8, 50)
    cut = bounds[13][0]                                                       # a chromosome end at a planted boundary
    bim = {"SNP": ["m%d" % i for i in range(L)], "Chr": ["1" if i < cut else "2" for i in range(L)], "Pos": [1000 * (i + 1) for i in range(L)]}
    for method in ("fourgamete", "spine"):
        res = r_api.HapBlocks(geno, method=method, map=bim)
        first, last, block_of = r_api.hap_blocks_host(host["recomb"], host["strong"], 50, np.asarray(bim["Chr"]), np.asarray(bim["Pos"]), None, method, 2)
        tab = res["blocks"]
        assert np.array_equal(tab["first"], first) and np.array_equal(tab["last"], last) and np.array_equal(res["block_of"], block_of)
        assert np.array_equal(res["counts"], host["counts"]) and np.array_equal(tab["n_markers"], last - first + 1)
        assert tab["chrom"] == ["1" if f < cut else "2" for f in first] and np.array_equal(tab["start"], 1000 * (first + 1))
        assert np.array_equal(tab["length"], 1000 * (last - first) + 1) and res["share"] == float((block_of >= 0).mean())
        rec = {(i, i + o) for i in range(L) for o in range(1, 51) if i + o < L and T.bit(host["recomb"], i, i + o)}
        strong = {(i, i + o) for i in range(L) for o in range(1, 51) if i + o < L and T.bit(host["strong"], i, i + o)}
        assert list(zip(first.tolist(), last.tolist())) == T.blocks_brute(rec, strong, L, 50, chrom=bim["Chr"], method=method)
        if method == "fourgamete":
            assert list(zip(first.tolist(), last.tolist())) == bounds and res["share"] == 1.0
    short = r_api.HapBlocks(geno, map=bim, kb=6)                              # 6 kb from a block's first marker: at most 7 markers
    assert short["blocks"]["n_markers"].max() == 7 and short["blocks"]["length"].max() <= 6001
    ld = r_api.HapLD(geno, window=50, map=bim)
    across = np.zeros((L, 50), dtype=bool)
    for o in range(1, 51):
        across[max(0, cut - o):cut, o - 1] = True
    want_def = (host["dprime"] > -2.0) & ~across
    assert np.array_equal(ld["defined"], want_def) and np.array_equal(ld["counts"], host["counts"])
    assert np.array_equal(ld["dprime"][want_def], host["dprime"][want_def]) and np.isnan(ld["dprime"][~want_def]).all()
    assert np.array_equal(ld["r2"][want_def], host["r2"][want_def]) and ld["mean_abs_dprime"].shape == (50,)
    assert abs(ld["mean_abs_dprime"][0] - np.abs(host["dprime"][:, 0][want_def[:, 0]]).mean()) <= 1e-12
    with pytest.raises(ValueError):
        r_api.HapLD(geno, kb=5)                                               # kb needs a map
    # the blocks as sets of the set test
    sets = r_api.sets_from_blocks(r_api.HapBlocks(geno, map=bim))
    assert [s.tolist() for s in sets["sets"]] == [list(range(f, e + 1)) for f, e in bounds]
    y, _ = synth.trait(Mt8, nqtl=3, beta=1.0, seed=5)
    out = r_api.SetTest(y, np.ones((n, 1)), geno, sets["sets"])
    assert len(out["p_skat"]) == len(bounds) and np.isfinite(out["p_skat"]).any() and (out["n_markers"] == [e - f + 1 for f, e in bounds]).all()
    rcpp_api.drop_cache()
