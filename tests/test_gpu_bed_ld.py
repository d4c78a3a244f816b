"""Pairwise-complete LD from a .bed file on the GPU: eagle_bed_ld_window / eagle_bed_ld_partners (k_bed_ld_pack, k_bedld_tile on the int8
MFMA, k_ld_partners) and LDPrune(bed=) / ImputeBed(ld_from="bed") on top.

Everything the device returns is compared with r_api.bed_ld_mask_host / bed_ld_partners_host on the same file -- the numpy restatements
that tests/test_bed_ld_host.py pins to a plain loop of the definition.  Mask words, pair counts and partners are integers, r2 is compared
bit for bit, files are bytes: every comparison is ==."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEAD = b"\x6c\x1b\x01"
# NB = floor((window + 31) / 32) + 1 = 2, 2, 2, 3, 4, 5, 6, 7, 8, 9, 9 block offsets: every group of two, a last group of one, and the seams
WINDOWS = (1, 31, 32, 33, 96, 97, 129, 161, 193, 225, 256)
_HOST = {}


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


def check(bed, n, L, window, t=0.2, l=8, min_r2=0.0, include=None, min_overlap=1, chrom=None, mem=8.0, codes=None):
    """Both calls against the host restatement; returns (mask, partners, r2)."""
    from eagleeverything_amd import r_api, rcpp_api
    codes = r_api.read_bed_codes(bed, (n, L)) if codes is None else codes
    key = (bed, window, t, l, min_r2, None if include is None else np.asarray(include).tobytes(), min_overlap,
           None if chrom is None else np.asarray(chrom).tobytes())
    if key not in _HOST:                                                       # one restatement per case, shared by the staging variants
        _HOST[key] = (r_api.bed_ld_mask_host(codes, window, t, include, min_overlap),
                      r_api.bed_ld_partners_host(codes, window, l, min_r2, include, min_overlap, chrom))
    want, (wp, wr) = _HOST[key]
    mask, npairs = rcpp_api.bed_ld_window(bed, (n, L), window, t, include, min_overlap, mem, return_pairs=True)
    assert mask.dtype == np.uint64 and mask.shape == want.shape
    assert np.array_equal(mask, want), (n, L, window, min_overlap, np.flatnonzero((mask != want).any(axis=1))[:10])
    assert npairs == int(np.unpackbits(np.ascontiguousarray(want).view(np.uint8)).sum())
    part, r2 = rcpp_api.bed_ld_partners(bed, (n, L), window, l, min_r2, include, min_overlap, chrom, mem, return_r2=True)
    assert part.dtype == np.int32 and part.shape == wp.shape and r2.dtype == np.float64
    assert np.array_equal(part, wp), (n, L, window, min_overlap, np.flatnonzero((part != wp).any(axis=1))[:10])
    assert np.array_equal(r2.view(np.uint64), wr.view(np.uint64)), (n, L, window)
    return mask, part, r2


# ------------------------------------------------------------------------------------------------ shapes at the kernel's edges
@pytest.mark.parametrize("n", [3, 127, 128, 129, 257])
def test_gpu_bed_ld_individuals_at_the_chunk_and_byte_edges(tmp_path, n):
    """The 128-individual K chunk, the 16-byte row tail, a last .bed byte with 1, 2 or 3 pad pairs; every window's block count."""
    L = 385
    Mt8, miss = panel(n, L, seed=100 + n, rate=0.05)
    bed = write_bed(tmp_path, "p", Mt8, miss)
    from eagleeverything_amd import r_api
    codes = r_api.read_bed_codes(bed, (n, L))
    for window in WINDOWS:
        mask, part, r2 = check(bed, n, L, window, l=5, codes=codes)
    assert mask.any() and (part[:, 0] >= 0).sum() > L // 2


@pytest.mark.parametrize("L", [1, 2, 127, 128, 129, 385])
def test_gpu_bed_ld_markers_at_the_tile_edges(tmp_path, L):
    """The 128-marker tile; windows wider than the panel."""
    n = 129
    Mt8, miss = panel(n, L, seed=200 + L, rate=0.05)
    bed = write_bed(tmp_path, "p", Mt8, miss)
    for window in (1, 33, 130, 256):
        mask, part, r2 = check(bed, n, L, window, l=32 if window == 256 else 3, chrom=(np.arange(L) >= 70).astype(np.int32))
    if L == 1:
        assert not mask.any() and (part == -1).all()


# ------------------------------------------------------------------------------------------------ missingness
def test_gpu_bed_ld_without_a_missing_code_is_the_panels_ld(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    n, L = 257, 300
    Mt8, _ = panel(n, L, seed=5, rate=0.0)
    Mt8[40], Mt8[41] = 1, 0                                                   # monomorphic
    bed = write_bed(tmp_path, "full", Mt8, None)
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(tmp_path))
    chrom = (np.arange(L) >= 170).astype(np.int32)
    for window, l in ((33, 7), (256, 32)):
        for mo in (1, n):
            mask, part, r2 = check(bed, n, L, window, l=l, min_overlap=mo, chrom=chrom)
            want, wp = rcpp_api.ld_window(geno["asciifileMt"], (n, L), window, 0.2, return_pairs=True)
            assert np.array_equal(mask, want) and wp > 0
            p2, r22 = rcpp_api.ld_partners(geno["asciifileMt"], (n, L), window, l, 0.0, chrom, return_r2=True)
            assert np.array_equal(part, p2) and np.array_equal(r2.view(np.uint64), r22.view(np.uint64))
    rcpp_api.drop_cache()


def test_gpu_bed_ld_heavy_missingness_and_degenerate_markers(tmp_path):
    from eagleeverything_amd import r_api
    n, L = 257, 300
    Mt8, miss = panel(n, L, seed=6, rate=0.6)
    miss[10, :] = True                                                        # no call at all
    miss[20, :] = True
    miss[20, 7] = False                                                       # called in a single individual
    # 30 and 31 are polymorphic overall, but 31 is constant over the individuals called at both: 31 varies only where 30 is missing
    Mt8[30] = np.where(np.arange(n) % 2 == 0, 1, -1)
    Mt8[31] = 1
    Mt8[31, :40] = -1
    miss[30], miss[31] = False, False
    miss[30, :40] = True
    bed = write_bed(tmp_path, "heavy", Mt8, miss)
    codes = r_api.read_bed_codes(bed, (n, L))
    for mo in (1, 5, n // 2):
        for window in (33, 256):
            mask, part, r2 = check(bed, n, L, window, l=6, min_overlap=mo, codes=codes)
    gone = [float((r_api.bed_ld_host(codes, 33, None, mo)[6][:-33] == -1.0).mean()) for mo in (1, 5, n // 2)]
    assert gone[0] <= gone[1] < 0.5 < gone[2]                                  # 0.4^2 n = 41 both-called on average: most pairs fall below n // 2
    assert (part[[10, 20]] == -1).all() and not np.isin(part, [10, 20]).any()
    mask1, part1, _ = check(bed, n, L, 5, t=0.0, l=10, codes=codes)
    assert not (int(mask1[30, 0]) & 1) and 31 not in part1[30] and 30 not in part1[31]      # not in LD, not a partner
    assert r_api.bed_ld_host(codes, 5)[6][30, 0] == -1.0 and (mask1[10] == 0).all() and (mask1[20] == 0).all()


def test_gpu_bed_ld_exact_tie_at_the_threshold(tmp_path):
    """r = 1/2 over fully called individuals: x_i = (+,+,+,+,-,-,-,-), x_j = (+,+,+,-,+,-,-,-) gives N = 8, D = 4, Si = Sj = 0, Q = 8:
    cov = 32, vi = vj = 64, cov^2 = 1024 = 0.25 * 4096 exactly.  Not in LD at 0.25 (strict >), in LD just below."""
    from eagleeverything_amd import r_api, rcpp_api
    xi = np.array([1, 1, 1, 1, -1, -1, -1, -1], dtype=np.int8)
    xj = np.array([1, 1, 1, -1, 1, -1, -1, -1], dtype=np.int8)
    n, L = 11, 2
    Mt8 = np.zeros((L, n), dtype=np.int8)
    Mt8[0, :8], Mt8[1, :8] = xi, xj
    miss = np.zeros((L, n), dtype=bool)
    miss[:, 8:] = True                                                        # three individuals without a call: N stays 8
    bed = write_bed(tmp_path, "tie", Mt8, miss)
    N, D, Si, Sj, Qi, Qj, r2 = r_api.bed_ld_host(r_api.read_bed_codes(bed, (n, L)), 1)
    assert (N[0, 0], D[0, 0], Si[0, 0], Sj[0, 0], Qi[0, 0], Qj[0, 0], r2[0, 0]) == (8, 4, 0, 0, 8, 8, 0.25)
    at, n_at = rcpp_api.bed_ld_window(bed, (n, L), 1, 0.25, return_pairs=True)
    below, n_below = rcpp_api.bed_ld_window(bed, (n, L), 1, float(np.nextafter(0.25, 0)), return_pairs=True)
    assert n_at == 0 and not at.any()
    assert n_below == 1 and below.tolist() == [[1], [0]]
    check(bed, n, L, 1, t=0.25)
    check(bed, n, L, 1, t=float(np.nextafter(0.25, 0)), min_r2=0.25)
    part, r2d = rcpp_api.bed_ld_partners(bed, (n, L), 1, 1, 0.25, return_r2=True)
    assert part.tolist() == [[1], [0]] and r2d.tolist() == [[0.25], [0.25]]                  # a candidate at r2 >= min_r2


# ------------------------------------------------------------------------------------------------ include and staging
def staging_windows(n, linc, window, mem, fidx=None, partners=False):
    """The windows of include/eagle_hip.h section 1b'''iv as (lo, hi) panel markers."""
    rb, ld = (n + 3) // 4, (n + 15) // 16 * 16
    S = max(1, int(min(64 * 2 ** 20, mem * 1e9 / 4) // rb))
    wmax = max(1024, 2 ** 27 // ld)
    if partners:
        wmax = min(wmax, max(1024, 2 ** 28 // (8 * window)))
    need, back = (2 * window + 1, 2 * window) if partners else (window + 1, window)
    f = np.arange(linc) if fidx is None else np.asarray(fidx)
    out, lo = [], 0
    while lo < linc:
        hi = min(linc, lo + wmax)
        hi = lo + int(np.searchsorted(f[lo:hi], f[lo] + S - 1, side="right"))
        hi = max(hi, min(linc, lo + need))
        out.append((lo, hi))
        lo = linc if hi >= linc else hi - back
    return out


def test_gpu_bed_ld_include_selects_the_panel(tmp_path):
    from eagleeverything_amd import r_api
    n, L = 129, 700
    Mt8, miss = panel(n, L, seed=9, rate=0.05)
    bed = write_bed(tmp_path, "inc", Mt8, miss)
    codes = r_api.read_bed_codes(bed, (n, L))
    rb = (n + 3) // 4
    hole = np.ones(L, dtype=bool)
    hole[150:450] = False                                                     # more excluded rows in a run than a staging window of 100 holds
    for include, mem in ((np.arange(L) % 2 == 0, 8.0), (np.arange(L) % 7 == 3, 8.0), (hole, 8.0), (hole, 4 * 100 * rb / 1e9)):
        linc = int(include.sum())
        chrom = (np.arange(linc) >= linc // 2).astype(np.int32)               # per PANEL marker
        for window in (33, 256):
            mask, part, r2 = check(bed, n, L, window, l=8, include=include, chrom=chrom, mem=mem, codes=codes)
            assert mask.shape[0] == linc and part.shape[0] == linc and part.max() < linc
    fidx = np.flatnonzero(hole)
    assert len(staging_windows(n, fidx.size, 33, 4 * 100 * rb / 1e9, fidx)) >= 3


def test_gpu_bed_ld_staging_windows_give_the_same_result(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    n, L = 257, 700
    rb = (n + 3) // 4
    Mt8, miss = panel(n, L, seed=10, rate=0.05)
    for a in (250, 299, 300, 560):                                            # copies across the rows where windows of 300 rows end
        Mt8[a + 1], Mt8[a - 20] = Mt8[a], -Mt8[a]
    bed = write_bed(tmp_path, "st", Mt8, miss)
    codes = r_api.read_bed_codes(bed, (n, L))
    every3 = np.arange(L) % 3 != 0
    small = 4 * 300 * rb / 1e9                                                # the library's arithmetic: a quarter of the budget, 300 rows
    assert len(staging_windows(n, L, 33, small)) >= 3 and len(staging_windows(n, L, 33, small, partners=True)) >= 3
    assert len(staging_windows(n, L, 33, 8.0)) == 1
    tiny = 4 * 1 * rb / 1e9                                                   # one row: every window is the least the call needs
    assert len(staging_windows(n, L, 33, tiny)) == L - 33 and len(staging_windows(n, int(every3.sum()), 33, small, np.flatnonzero(every3))) >= 3
    for include in (None, every3):
        for window in (33, 256):
            one = check(bed, n, L, window, l=8, include=include, codes=codes)
            for mem in (small, tiny) if window == 33 else (small,):
                got = check(bed, n, L, window, l=8, include=include, mem=mem, codes=codes)
                assert all(np.array_equal(a, b) for a, b in zip(one, got))


# ------------------------------------------------------------------------------------------------ end to end
def test_gpu_ldprune_from_the_bed_file_end_to_end(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    n, L, window, t = 129, 600, 50, 0.2
    Mt8, miss = panel(n, L, seed=21, rate=0.1)
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
    want_mask = r_api.bed_ld_mask_host(codes, window, t, idx, max(2, n // 10))
    keep = np.flatnonzero(r_api.ld_prune_keep(want_mask, window))
    assert 0 < keep.size < idx.size
    msgs = []
    pruned = r_api.LDPrune(flt, window=window, r2=t, bed=str(src / "panel"), outdir=str(tmp_path / "ld"), message=msgs.append)
    assert np.array_equal(pruned["marker_index"], idx[keep]) and list(pruned["dim_of_ascii_M"]) == [n, keep.size]
    ref = tmp_path / "ref"
    ref.mkdir()
    rcpp_api.filter_markers(flt["asciifileM"], flt["asciifileMt"], flt["dim_of_ascii_M"], keep, str(ref / "M.ascii"), str(ref / "Mt.ascii"))
    for name, key in (("M.ascii", "asciifileM"), ("Mt.ascii", "asciifileMt")):
        assert open(pruned[key], "rb").read() == open(str(ref / name), "rb").read()
    # the panel's own LD (missing = heterozygous) prunes differently: bed= is what changed the answer
    plain = r_api.LDPrune(flt, window=window, r2=t, outdir=str(tmp_path / "ld_plain"))
    assert not np.array_equal(plain["marker_index"], pruned["marker_index"])
    # a .fam of another size is refused
    other = tmp_path / "other"
    other.mkdir()
    write_bed(other, "panel", Mt8[:, :100], miss[:, :100])
    said = []
    assert r_api.LDPrune(flt, window=window, r2=t, bed=str(other / "panel"), outdir=str(tmp_path / "ld2"), message=said.append) is None
    assert any("100 individuals" in s_ for s_ in said) and any("terminated with errors" in s_ for s_ in said)
    rcpp_api.drop_cache()


def test_gpu_impute_bed_with_partners_from_the_bed_file(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    n, L, k, l = 64, 300, 5, 4
    Mt8, miss = panel(n, L, seed=31, rate=0.15)
    src = tmp_path / "src"
    src.mkdir()
    bed = write_bed(src, "panel", Mt8, miss)
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(src))
    codes = r_api.read_bed_codes(bed, (n, L))
    ingested = np.array([-1, 0, 0, 1], dtype=np.int8)[codes]
    p_bed, _ = r_api.bed_ld_partners_host(codes, 50, l, 0.0, None, max(2, n // 10))
    p_panel, _ = r_api.ld_partners_host(ingested, 50, l, 0.0)
    assert not np.array_equal(p_bed, p_panel)
    rows_bed, counts_bed = r_api.impute_ldknn_host(codes, p_bed, k, 1, 4)
    rows_panel, _ = r_api.impute_ldknn_host(codes, p_panel, k, 1, 4)
    res = r_api.ImputeBed(bed, geno, str(tmp_path / "a" / "p"), k=k, local=l, ld_from="bed")
    assert np.array_equal(res["partners"], p_bed) and np.array_equal(res["counts"], counts_bed)
    assert open(res["bed"], "rb").read() == HEAD + rows_bed.tobytes()
    dflt = r_api.ImputeBed(bed, geno, str(tmp_path / "b" / "p"), k=k, local=l)             # the defaults: the panel's LD, as before
    assert np.array_equal(dflt["partners"], p_panel) and open(dflt["bed"], "rb").read() == HEAD + rows_panel.tobytes()
    work = tmp_path / "work"
    work.mkdir()
    g2 = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(work), impute=k, impute_local=l, impute_ld_from="bed")
    # ReadMarker gives the .bim file's chromosomes (one here), which changes nothing
    assert open(os.path.join(str(work), "imputed", "panel.bed"), "rb").read() == HEAD + rows_bed.tobytes() and g2["dim_of_ascii_M"] == [n, L]
    rcpp_api.drop_cache()
