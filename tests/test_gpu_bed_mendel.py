"""Mendel errors and parentage assignment on the GPU from the .bed file: eagle_bed_mendel and eagle_bed_parentage (k_ibd_planes_bed, then
the kernels of eagle_mendel.hip with the called plane), which still know the missing calls -- a child that is not called has no error, a
parent that is not called can pass either allele, and a candidate's overlap counts the markers called in all three -- and r_api.Mendel /
r_api.Parentage on top of both routes.

The device's tables are compared with r_api.mendel_host / r_api.parentage_host on r_api.ibd_genotypes_bed(read_bed_codes(...)) -- the
numpy restatements that tests/test_mendel_host.py pins to plain loops over allele sets (include/eagle_hip.h section 1b'''viii) -- and, on
a file without a missing code, with the ingested panel's route.  Everything is integers: every comparison is ==."""
import numpy as np
import pytest

import mendel_truth as T
from test_gpu_bed_ibd import panel_of
from test_gpu_bed_ld_stats import write_bed              # pad bit pairs of a row's last byte set to 01 and 11
from test_gpu_mendel import (LS, N_D, N_O, N_S, NS, TS, assignment_panel, candidate_lists, edge_markers, kinds_panel, random_panel, same_rows,
                             trio_list)

pytestmark = pytest.mark.gpu

SMALL_GB = 1e-4                                          # staging windows of 25,000 bytes: 757 rows at n = 129
TINY_GB = 2e-5                                           # 5,000 bytes


@pytest.mark.parametrize("n", NS)
def test_gpu_bed_mendel_equals_host_at_word_and_wave_edges(tmp_path, n):
    from eagleeverything_amd import r_api, rcpp_api
    errors = hidden = 0
    for L in LS:
        g, called = random_panel(n, L, seed=300 * n + L, miss=0.1)
        bed = write_bed(tmp_path, "p%d" % L, g, ~called)
        gg, cc = r_api.ibd_genotypes_bed(r_api.read_bed_codes(bed, (n, L)))
        assert np.array_equal(cc, called) and np.array_equal(gg, g)
        for count in TS:
            trios = trio_list(n, count, seed=n + L + count)
            want_tab, want_marker = r_api.mendel_host(gg, cc, trios)
            tab, marker = rcpp_api.bed_mendel(bed, (n, L), trios)
            same_rows(tab, want_tab, (n, L, count, "trio"))
            same_rows(marker, want_marker, (n, L, count, "marker"))
            errors += int(tab[:, 5].sum())
            hidden += int(not np.array_equal(want_tab, r_api.mendel_host(gg, None, trios)[0]))
        only, none = rcpp_api.bed_mendel(bed, (n, L), trios, markers=False)
        assert none is None
        same_rows(only, want_tab, (n, L, "without the marker counts"))
    assert errors > 0 and hidden > 0                     # the missing calls matter: as hets they give other tables
    rcpp_api.drop_cache()


@pytest.mark.parametrize("L", (65, 129, 1000))
def test_gpu_bed_mendel_every_error_kind_and_errors_that_missing_calls_remove(tmp_path, L):
    from eagleeverything_amd import r_api, rcpp_api
    g, called, trios = kinds_panel(L, True)
    edges = edge_markers(L)
    bed = write_bed(tmp_path, "k", g, ~called)
    tab, marker = rcpp_api.bed_mendel(bed, (64, L), trios)
    want = r_api.mendel_host(g, called, trios)
    same_rows(tab, want[0], "trio")
    same_rows(marker, want[1], "marker")
    assert (tab[:, 5] == len(edges)).all() and (marker[edges] == 16).all() and marker.sum() == 16 * len(edges)      # all 16 kinds, everywhere
    if L == 65:
        loops = T.mendel_loops(g, called, trios.tolist())
        assert np.array_equal(tab, loops[0]) and np.array_equal(marker, loops[1])
    # the child's call goes missing at every planted marker of the even trios: their errors disappear
    g2, called2 = g.copy(), called.copy()
    for c in trios[::2, 0].tolist():
        called2[edges, c] = False
        g2[edges, c] = 0
    bed2 = write_bed(tmp_path, "k2", g2, ~called2)
    tab2, marker2 = rcpp_api.bed_mendel(bed2, (64, L), trios)
    want2 = r_api.mendel_host(g2, called2, trios)
    same_rows(tab2, want2[0], "trio, child not called")
    same_rows(marker2, want2[1], "marker, child not called")
    assert (tab2[::2, 5] == 0).all() and np.array_equal(tab2[1::2], tab[1::2]) and (marker2[edges] == 8).all()
    assert (tab2[::2, 0] <= L - len(edges)).all()        # and the overlaps shrink with them
    rcpp_api.drop_cache()


@pytest.mark.parametrize("n", (65, 129))
def test_gpu_bed_mendel_include_and_small_windows(tmp_path, n):
    """The panel is a selection of the file's markers (which moves every word edge of the panel off the file's), staged in several windows."""
    from eagleeverything_amd import r_api, rcpp_api
    L = 2100
    g, called = random_panel(n, L, seed=n, miss=0.05)
    bed, Lf, inc = panel_of(tmp_path, "m", g, called, L + L // 6, seed=n)
    codes = r_api.read_bed_codes(bed, (n, Lf))
    gg, cc = r_api.ibd_genotypes_bed(codes[inc])
    assert np.array_equal(cc, called) and np.array_equal(gg, g)
    trios = trio_list(n, 130, seed=n)
    want = r_api.mendel_host(g, called, trios)
    off, sires, dams = trios[:5, 0].copy(), np.arange(0, n, 2, dtype=np.int32), np.arange(n - 1, 0, -3, dtype=np.int32)
    off = np.unique(off)
    wantp = r_api.parentage_host(g, called, off, sires, dams, 1800)         # 0.95^3 L = 1,800: about half of the candidates
    assert (wantp[:, :, 3] >= 1800).all() and wantp[:, :, 3].max() < L
    for mem in (8.0, SMALL_GB, TINY_GB):
        tab, marker = rcpp_api.bed_mendel(bed, (n, Lf), trios, inc, mem)
        same_rows(tab, want[0], (mem, "trio"))
        same_rows(marker, want[1], (mem, "marker"))
        same_rows(rcpp_api.bed_parentage(bed, (n, Lf), off, sires, dams, inc, 1800, False, mem), wantp, (mem, "parentage"))
    rcpp_api.drop_cache()


@pytest.mark.parametrize("n_o", N_O)
def test_gpu_bed_parentage_equals_host_at_tile_edges(tmp_path, n_o):
    from eagleeverything_amd import r_api, rcpp_api
    g, called, trios = assignment_panel(0.1)
    L, n = g.shape
    bed = write_bed(tmp_path, "a", g, ~called)
    seen = set()
    for n_s in N_S + (0,):
        for n_d in N_D:
            if n_s == 0 and n_d == 0:
                continue
            off, sires, dams = candidate_lists(n, trios, n_o, n_s, n_d, seed=n_s + n_d)
            selfing = (n_s + n_d) % 2 == 1
            for mo in (1, 200):                          # about 0.9^3 L = 219 markers are called in all three: 200 cuts some candidates out
                want = r_api.parentage_host(g, called, off, sires, dams, mo, selfing)
                got = rcpp_api.bed_parentage(bed, (n, L), off, sires, dams, None, mo, selfing)
                same_rows(got, want, (n_o, n_s, n_d, mo, selfing))
                seen.update(got[:, :, 3].ravel().tolist())
                if mo == 200:
                    assert (got[:, :, 3][got[:, :, 3] >= 0] >= 200).all()
    assert len(seen - {-1}) >= 3 and -1 in seen                # the overlaps differ from candidate to candidate; some rows have no candidate
    rcpp_api.drop_cache()


def test_gpu_bed_parentage_min_overlap_cuts_the_true_parent_out(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    g, called, trios = assignment_panel(0.0)
    L, n = g.shape
    c, f, m = trios[0].tolist()
    g, called = g.copy(), called.copy()
    called[::3, f] = False                               # the true father is called at two markers of three
    g[::3, f] = 0
    bed = write_bed(tmp_path, "o", g, ~called)
    sires = np.asarray([f] + [i for i in range(20) if i != f], dtype=np.int32)
    dams = np.asarray([m] + [i for i in range(75, 95) if i != m], dtype=np.int32)
    ov = int(np.count_nonzero(called[:, f]))
    assert ov == 200
    got = rcpp_api.bed_parentage(bed, (n, L), [c], sires, dams, None, ov)
    same_rows(got, r_api.parentage_host(g, called, [c], sires, dams, ov), "at the overlap")
    assert got[0, 0].tolist() == [f, m, 0, ov]
    cut = rcpp_api.bed_parentage(bed, (n, L), [c], sires, dams, None, ov + 1)
    same_rows(cut, r_api.parentage_host(g, called, [c], sires, dams, ov + 1), "one above the overlap")
    assert f not in cut[0, :, 0] and (cut[0, :, 3] == L).all() and cut[0, 0, 2] > 0
    # single-parent assignment: the overlap is that of the child and the one known parent
    one = rcpp_api.bed_parentage(bed, (n, L), [c], sires, None, None, ov)
    same_rows(one, r_api.parentage_host(g, called, [c], sires, None, ov), "single parent")
    assert one[0, 0].tolist() == [f, -1, 0, ov]
    assert f not in rcpp_api.bed_parentage(bed, (n, L), [c], sires, None, None, ov + 1)[0, :, 0]
    rcpp_api.drop_cache()


def test_gpu_bed_routes_without_missing_are_the_ingested_panel(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    g, called, trios = assignment_panel(0.0)
    L, n = g.shape
    bed = write_bed(tmp_path, "full", g, ~called)
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(tmp_path))
    assert list(geno["dim_of_ascii_M"]) == [n, L]
    rng = np.random.default_rng(3)
    lst = np.concatenate((trios, np.stack([trios[:, 0], rng.permutation(75)[:60], trios[:, 2]], axis=1))).astype(np.int32)
    a = rcpp_api.bed_mendel(bed, (n, L), lst, None, SMALL_GB)
    b = rcpp_api.mendel(geno["asciifileM"], (n, L), lst)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0][60:, 5].sum() > 0 and a[0][:60, 5].sum() == 0
    off, sires, dams = candidate_lists(n, trios, 5, 65, 130, seed=1)
    a = rcpp_api.bed_parentage(bed, (n, L), off, sires, dams, None, 1, False, SMALL_GB)
    b = rcpp_api.parentage(geno["asciifileM"], (n, L), off, sires, dams)
    assert a.tobytes() == b.tobytes() and (a[:, 0, 3] == L).all()
    rcpp_api.drop_cache()


def test_gpu_Mendel_and_Parentage_end_to_end_on_a_written_fileset(tmp_path):
    """r_api.Mendel(fam=...) and r_api.Parentage(...) on a fileset whose .fam records the pedigree, three fathers wrongly; both routes."""
    from eagleeverything_amd import r_api, rcpp_api
    g, called, trios = T.pedigree(30, 40, 500, seed=8, miss=0.03)
    L, n = g.shape
    recorded = trios.copy()
    recorded[[3, 17, 30], 1] = [(f + 1) % 15 for f in recorded[[3, 17, 30], 1]]          # another founder sire
    recorded[5, 2] = -1                                                                     # an unrecorded mother
    bed = write_bed(tmp_path, "ped", g, ~called)
    names = ["id%d" % i for i in range(n)]
    rows = {int(c): (f, m) for c, f, m in recorded.tolist()}
    with open(str(tmp_path / "ped.fam"), "w") as fh:
        for i in range(n):
            f, m = rows.get(i, (-1, -1))
            fh.write("F %s %s %s %d -9\n" % (names[i], names[f] if f >= 0 else "0", names[m] if m >= 0 else "0", 1 + i % 2))
    prefix = str(tmp_path / "ped")
    assert np.array_equal(r_api.fam_trios(prefix + ".fam"), recorded)
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(prefix, type="PLINKbed", outdir=str(tmp_path))
    map = r_api.ReadBim(prefix + ".bim")
    for route, cm in ((dict(fam=prefix + ".fam"), None), (dict(bed=prefix), called)):
        res = r_api.Mendel(geno, map=map, **route)
        tab, marker = r_api.mendel_host(g, cm, recorded)
        ref = r_api.mendel_summary(recorded, tab, marker, n)
        assert sorted(res) == sorted(list(ref) + ["SNP"]) and res["SNP"] == list(map["SNP"])
        for k in ref:
            assert np.array_equal(res[k], ref[k], equal_nan=res[k].dtype.kind == "f"), k
        assert set(np.argsort(res["errors"])[-3:].tolist()) == {3, 17, 30} and res["errors_as_child"][recorded[3, 0]] == res["errors"][3]
        keep = r_api.mendel_keep_mask(res["marker_errors"], recorded.shape[0], 0.05)
        assert keep.shape == (L,) and keep.sum() > L // 2
        # who are the parents of the three?  Everybody but the offspring's own descendants' noise: all founders as candidates
        off = recorded[[3, 17, 30], 0]
        par = r_api.Parentage(geno, off, np.arange(15), np.arange(15, 30), min_overlap=100, max_rate=0.01, **({} if cm is None else dict(bed=prefix)))
        want = r_api.parentage_summary(off, r_api.parentage_host(g, cm, off, np.arange(15), np.arange(15, 30), 100), 0.01)
        for k in want:
            assert np.array_equal(par[k], want[k], equal_nan=want[k].dtype.kind == "f"), k
        founders = trios[[3, 17, 30], 1] < 30
        assert np.array_equal(par["sire"][founders], trios[[3, 17, 30], 1][founders]) and par["assigned"][founders].all()
    with pytest.raises(ValueError):
        r_api.Mendel(geno)                               # no trios, no fam, no bed
    rcpp_api.drop_cache()
