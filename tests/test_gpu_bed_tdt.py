"""The transmission disequilibrium test on the GPU from the .bed file: eagle_bed_tdt (k_ibd_planes_bed, then the kernels of eagle_tdt.hip
with the called plane and the max(T) tile), which still knows the missing calls -- a trio with a missing call at a marker is not complete
there -- and r_api.TDT on top of both routes.

The device's words are compared with r_api.tdt_host on r_api.ibd_genotypes_bed(read_bed_codes(...)) -- the numpy restatement that
tests/test_tdt_host.py pins to plain loops over allele choices (include/eagle_hip.h section 1b''''viii) -- and, on a file without a
missing code, with the ingested panel's route.  Every comparison is ==."""
import numpy as np
import pytest

import mendel_truth as M
import tdt_truth as T
from test_gpu_bed_ibd import panel_of
from test_gpu_bed_ld_stats import write_bed              # pad bit pairs of a row's last byte set to 01 and 11
from test_gpu_mendel import LS, NS, TS, trio_list
from test_gpu_tdt import sib_panel

pytestmark = pytest.mark.gpu

SMALL_GB = 1e-4                                          # staging windows of 25,000 bytes: 757 rows at n = 129
TINY_GB = 2e-5                                           # 5,000 bytes


@pytest.mark.parametrize("n", NS)
def test_gpu_bed_tdt_counts_equal_host_at_word_and_wave_edges(tmp_path, n):
    from eagleeverything_amd import r_api, rcpp_api
    informative = hidden = 0
    for L in LS:
        rng = np.random.default_rng(300 * n + L)
        g = rng.integers(-1, 2, (L, n)).astype(np.int8)
        called = rng.random((L, n)) >= 0.1
        g[L - 1, [2, 0, 1]], called[L - 1, [2, 0, 1]] = (0, 0, -1), True     # a het father passes A2 on the last marker
        g[~called] = 0
        bed = write_bed(tmp_path, "p%d" % L, g, ~called)
        gg, cc = r_api.ibd_genotypes_bed(r_api.read_bed_codes(bed, (n, L)))
        assert np.array_equal(cc, called) and np.array_equal(gg, g)
        for count in TS:
            trios = trio_list(n, count, seed=n + L + count)
            want = r_api.tdt_host(gg, cc, trios)
            got = rcpp_api.bed_tdt(bed, (n, L), trios)
            T.same(got, want, (n, L, count))
            assert got["marker"][L - 1, 0] >= 1
            informative += int(got["trio"][:, 1:3].sum())
            hidden += int(not np.array_equal(want["trio"], r_api.tdt_host(gg, None, trios)["trio"]))
    assert informative > 0 and hidden > 0                # the missing calls matter: as hets they give other tables
    rcpp_api.drop_cache()


@pytest.mark.parametrize("L", (65, 129, 1000))
def test_gpu_bed_tdt_every_informative_and_error_kind_and_what_missing_calls_remove(tmp_path, L):
    from eagleeverything_amd import r_api, rcpp_api
    g, called, trios = T.kinds_panel(L, True)
    edges = T.edge_markers(L)
    bed = write_bed(tmp_path, "k", g, ~called)
    got = rcpp_api.bed_tdt(bed, (84, L), trios, seed=L, R=33)
    T.same(got, r_api.tdt_host(g, called, trios, seed=L, R=33), "kinds")
    table = T.triple_table()
    per_marker = np.sum([table[t][:5] for t in T.informative_triples()], axis=0)
    assert (got["marker"][edges] == per_marker).all() and got["marker"][edges].sum(axis=1).min() >= 11      # the 11 kinds, and nothing from the 16 errors
    assert (got["trio"][11:, 0] <= L - len(edges)).all()                                                     # an error is not complete
    if L == 65:
        T.same(got, T.tdt_loops(g, called, trios, seed=L, R=33), "loops")
    # the child's call goes missing at every planted marker of the even trios: their transmissions disappear
    g2, called2 = g.copy(), called.copy()
    for c in trios[:11:2, 0].tolist():
        called2[edges, c] = False
        g2[edges, c] = 0
    bed2 = write_bed(tmp_path, "k2", g2, ~called2)
    got2 = rcpp_api.bed_tdt(bed2, (84, L), trios)
    T.same(got2, r_api.tdt_host(g2, called2, trios), "child not called")
    odd = np.sum([table[t][:5] for t in T.informative_triples()[1::2]], axis=0)
    assert (got2["marker"][edges] == odd).all() and np.array_equal(got2["trio"][1:11:2], got["trio"][1:11:2])
    rcpp_api.drop_cache()


@pytest.mark.parametrize("n", (65, 129))
def test_gpu_bed_tdt_include_and_small_windows(tmp_path, n):
    """The panel is a selection of the file's markers (which moves every word edge of the panel off the file's), staged in several windows."""
    from eagleeverything_amd import r_api, rcpp_api
    L = 2100
    rng = np.random.default_rng(n)
    g = rng.integers(-1, 2, (L, n)).astype(np.int8)
    called = rng.random((L, n)) >= 0.1
    g[~called] = 0
    bed, Lf, inc = panel_of(tmp_path, "m", g, called, L + L // 6, seed=n)
    codes = r_api.read_bed_codes(bed, (n, Lf))
    gg, cc = r_api.ibd_genotypes_bed(codes[inc])
    assert np.array_equal(cc, called) and np.array_equal(gg, g)
    trios = trio_list(n, 130, seed=n)
    want = r_api.tdt_host(g, called, trios, seed=n, first=2, R=40)
    for mem in (8.0, SMALL_GB, TINY_GB):
        T.same(rcpp_api.bed_tdt(bed, (n, Lf), trios, inc, None, n, 2, 40, mem), want, mem)
    assert want["marker"].sum() > 0 and want["count1"].sum() > 0 and want["count1"].max() <= 40
    rcpp_api.drop_cache()


def test_gpu_bed_tdt_without_missing_is_the_ingested_panel(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    g, trios = sib_panel(30, 100, 300, seed=5)
    n, L = g.shape[1], 300
    bed = write_bed(tmp_path, "full", g, np.zeros(g.shape, dtype=bool))
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(tmp_path))
    assert list(geno["dim_of_ascii_M"]) == [n, L]
    a = rcpp_api.bed_tdt(bed, (n, L), trios, None, None, 3, 1, 64, SMALL_GB)
    b = rcpp_api.tdt(geno["asciifileM"], (n, L), trios, None, 3, 1, 64)
    T.same(a, b, "the two routes")
    assert a["marker"].sum() > 0 and a["trio"][:, 0].max() == L
    rcpp_api.drop_cache()


def test_gpu_TDT_end_to_end_on_a_written_fileset(tmp_path):
    """r_api.TDT(fam=...) and r_api.TDT(bed=...) on a fileset whose .fam records the pedigree and the phenotypes; both routes."""
    from eagleeverything_amd import r_api, rcpp_api
    g, called, trios = M.pedigree(30, 40, 500, seed=8, miss=0.03)
    L, n = g.shape
    bed = write_bed(tmp_path, "ped", g, ~called)
    names = ["id%d" % i for i in range(n)]
    rows = {int(c): (f, m) for c, f, m in trios.tolist()}
    pheno = ["2" if i >= 30 and i % 3 else "1" for i in range(n)]
    with open(str(tmp_path / "ped.fam"), "w") as fh:
        for i in range(n):
            f, m = rows.get(i, (-1, -1))
            fh.write("F %s %s %s %d %s\n" % (names[i], names[f] if f >= 0 else "0", names[m] if m >= 0 else "0", 1 + i % 2, pheno[i]))
    prefix = str(tmp_path / "ped")
    assert np.array_equal(r_api.fam_trios(prefix + ".fam"), trios)
    used = trios[[p == "2" for p in np.asarray(pheno)[trios[:, 0]]]]
    assert 0 < used.shape[0] < trios.shape[0]
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(prefix, type="PLINKbed", outdir=str(tmp_path))
    map = r_api.ReadBim(prefix + ".bim")
    for route, cm in ((dict(fam=prefix + ".fam"), None), (dict(bed=prefix), called)):
        res = r_api.TDT(geno, map=map, R=40, seed=9, **route)
        ref = r_api.tdt_summary(r_api.tdt_host(g, cm, used, seed=9, R=40))
        assert sorted(res) == sorted(list(ref) + ["SNP", "trios"]) and res["SNP"] == list(map["SNP"]) and np.array_equal(res["trios"], used)
        for k in ref:
            assert np.array_equal(res[k], ref[k], equal_nan=True), k
        # affected= overrides the phenotypes of the .fam
        everybody = r_api.TDT(geno, affected=np.ones(n, dtype=bool), **route)
        assert np.array_equal(everybody["marker"], r_api.tdt_host(g, cm, trios)["marker"]) and everybody["R"] == 0
    with pytest.raises(ValueError):
        r_api.TDT(geno, fam=prefix + ".fam", affected=np.zeros(n, dtype=bool))
    rcpp_api.drop_cache()
