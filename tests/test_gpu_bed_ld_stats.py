"""LD scores and the LD decay curve from a .bed file on the GPU: eagle_bed_ld_stats (k_bed_ld_pack, k_bedld_tile's r2 mode on the int8
MFMA, k_ld_reduce) and LDScore(bed=) / LDDecay(bed=) on top.

The device's sums are compared with r_api.ld_stats_host(r_api.bed_ld_host(...)[6], ...) on the same file -- the numpy restatements that
tests/test_bed_ld_host.py and tests/test_ld_stats_host.py pin to plain loops of the definitions (include/eagle_hip.h sections 1b'''iv and
1b'''v).  Everything is an integer: every comparison is ==."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

PREFIX = os.path.join(GOLDEN, "plink_150x100")
WINDOWS = (1, 33, 256)


def write_bed(tmp_path, name, Mt8, miss):
    """A fileset with `miss` as the missing code and the pad bit pairs of every row's last byte set to 01 (missing) and 11 (hom A2)."""
    from eagleeverything_amd import synth
    L, n = Mt8.shape
    bed = synth.write_bed(str(tmp_path / name), Mt8, missing=miss)
    if n % 4:
        rb = (n + 3) // 4
        raw = bytearray(open(bed, "rb").read())
        pad = (0b11011101 << (2 * (n % 4))) & 0xff
        for m in range(L):
            raw[3 + m * rb + rb - 1] |= pad
        open(bed, "wb").write(bytes(raw))
    return bed


def panel(n, L, seed, rate):
    """Correlated runs of markers (every marker is, with probability 0.6, its predecessor with a tenth of the genotypes redrawn) with
    `rate` missing at random."""
    rng = np.random.default_rng(seed)
    Mt8 = rng.integers(-1, 2, size=(L, n)).astype(np.int8)
    for j in range(1, L):
        if rng.random() < 0.6:
            Mt8[j] = np.where(rng.random(n) < 0.1, Mt8[j], Mt8[j - 1])
    return Mt8, rng.random((L, n)) < rate


def pos_of(L):
    return (np.arange(L, dtype=np.int64) * 1000 + np.where(np.arange(L) % 7 == 3, 2500, 0)).astype(np.int64)


def variants(linc, window):
    chrom = (np.arange(linc) >= linc // 2).astype(np.int32)                   # per PANEL marker
    pos = pos_of(linc)
    return (dict(),
            dict(chrom=chrom, edges=np.arange(1, window + 2)),
            dict(pos=pos, max_dist=20000, edges=[1500, 3000, 9000, 15000]),
            dict(chrom=chrom, pos=pos, edges=np.arange(513) * 45))


def same(got, want, what):
    assert len(got) == len(want), what
    for g, w, dt in zip(got, want, (np.uint64, np.int32, np.uint64, np.int64)):
        assert g.dtype == dt and g.shape == w.shape, what
        assert np.array_equal(g, w), (what, np.flatnonzero(g != w)[:10])


def check(bed, n, L, codes, include=None, min_overlap=1):
    from eagleeverything_amd import r_api, rcpp_api
    linc = L if include is None else int(np.asarray(include).sum())
    for window in WINDOWS:
        band = r_api.bed_ld_host(codes, window, include, min_overlap)[6]
        assert band.shape == (linc, window)
        for kw in variants(linc, window):
            got = rcpp_api.bed_ld_stats(bed, (n, L), window, include, min_overlap, **kw)
            same(got, r_api.ld_stats_host(band, **kw), (n, L, window, min_overlap, sorted(kw)))
    return got


def test_gpu_bed_ld_stats_golden_fileset():
    from eagleeverything_amd import r_api
    n, L = 150, 100
    codes = r_api.read_bed_codes(PREFIX, (n, L))
    got = check(PREFIX + ".bed", n, L, codes)
    assert got[0].any() and got[3].sum() > 0
    check(PREFIX + ".bed", n, L, codes, include=np.arange(L) % 2 == 0, min_overlap=20)


@pytest.mark.parametrize("min_overlap", [1, 20])
def test_gpu_bed_ld_stats_missing_codes_and_include(tmp_path, min_overlap):
    from eagleeverything_amd import r_api
    n, L = 65, 300
    Mt8, miss = panel(n, L, seed=41, rate=0.10)
    miss[10, :] = True                                                        # no call at all: no pair, score 1.0
    bed = write_bed(tmp_path, "p", Mt8, miss)
    codes = r_api.read_bed_codes(bed, (n, L))
    U, cnt = check(bed, n, L, codes, min_overlap=min_overlap)[:2]
    assert U[10] == 0 and cnt[10] == 0 and U.any()
    check(bed, n, L, codes, include=np.arange(L) % 2 == 0, min_overlap=min_overlap)


@pytest.mark.parametrize("every", [1, 3])
def test_gpu_bed_ld_stats_staging_windows_give_the_same_result(tmp_path, every):
    """Windows of 100 file rows (a quarter of the budget, the library's arithmetic) against the one window of the default budget."""
    from eagleeverything_amd import rcpp_api
    from test_gpu_bed_ld import staging_windows
    n, L = 129, 700
    rb = (n + 3) // 4
    small = 4 * 100 * rb / 1e9
    Mt8, miss = panel(n, L, seed=44, rate=0.05)
    bed = write_bed(tmp_path, "st", Mt8, miss)
    include = None if every == 1 else np.arange(L) % every != 0
    fidx = None if include is None else np.flatnonzero(include)
    linc = L if include is None else fidx.size
    for window in (1, 33):
        assert len(staging_windows(n, linc, window, small, fidx, partners=True)) >= 3
        assert len(staging_windows(n, linc, window, 8.0, fidx, partners=True)) == 1
        for kw in variants(linc, window):
            one = rcpp_api.bed_ld_stats(bed, (n, L), window, include, 1, **kw)
            same(rcpp_api.bed_ld_stats(bed, (n, L), window, include, 1, availmemGb=small, **kw), one, (every, window, sorted(kw)))


def test_gpu_bed_ld_stats_without_a_missing_code_is_the_panels(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    n, L = 257, 300
    Mt8, _ = panel(n, L, seed=5, rate=0.0)
    Mt8[40], Mt8[41] = 1, 0                                                   # monomorphic
    bed = write_bed(tmp_path, "full", Mt8, None)
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(tmp_path))
    for window in WINDOWS:
        for kw in variants(L, window):
            for mo in (1, n):
                same(rcpp_api.bed_ld_stats(bed, (n, L), window, None, mo, **kw), rcpp_api.ld_stats(geno["asciifileMt"], (n, L), window, **kw),
                     (window, mo, sorted(kw)))
    # the interface: bed= selects the pairwise-complete source, and here both sources agree
    a, b = r_api.LDScore(geno, window=33), r_api.LDScore(geno, window=33, bed=bed)
    assert all(np.array_equal(a[k], b[k]) for k in ("score", "partners", "u")) and a["score"][40] == 1.0 and a["score"].max() > 2.0
    a, b = r_api.LDDecay(geno, window=33), r_api.LDDecay(geno, window=33, bed=bed, min_overlap=n)
    assert all(np.array_equal(a[k], b[k]) for k in ("edges", "pairs", "sum")) and a["half_decay"] == b["half_decay"]
    rcpp_api.drop_cache()


def test_gpu_ldscore_from_the_bed_file_of_a_filtered_panel(tmp_path):
    """include= defaults to the geno dict's marker_index, as LDPrune(bed=) takes it."""
    from eagleeverything_amd import r_api, rcpp_api
    n, L = 65, 300
    Mt8, miss = panel(n, L, seed=43, rate=0.10)
    Mt8[::5] = np.where(np.random.default_rng(3).random((len(Mt8[::5]), n)) < 0.1, 1, -1)     # every fifth marker: maf 0.1, filtered out
    src = tmp_path / "src"
    src.mkdir()
    bed = write_bed(src, "panel", Mt8, miss)
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(src))
    flt = r_api.FilterMarkers(geno, maf=0.25, bed=bed, outdir=str(tmp_path / "qc"))
    idx = np.asarray(flt["marker_index"])
    assert 0.2 * L < idx.size < L
    codes = r_api.read_bed_codes(bed, (n, L))
    mo = 7
    U, cnt = r_api.ld_stats_host(r_api.bed_ld_host(codes, 50, idx, mo)[6])
    res = r_api.LDScore(flt, bed=str(src / "panel"), min_overlap=mo)
    assert np.array_equal(res["u"], U) and np.array_equal(res["partners"], cnt) and res["u"].size == idx.size
    panel_only = r_api.LDScore(flt)                                           # missing = heterozygous: another answer
    assert not np.array_equal(panel_only["u"], U)
    with pytest.raises(ValueError):
        r_api.LDScore(flt, bed=str(src / "panel"), include=np.arange(L) % 2 == 0)      # not the panel's markers
    rcpp_api.drop_cache()
