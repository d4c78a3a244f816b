"""Linkage disequilibrium on the GPU: eagle_ld_window / eagle_ld_dots (k_ld_tile on the int8 MFMA, band and picks mode) and the
interface on top (r_api.LDPrune, r_api.LDofLoci, am.tag_markers).

Expected values are numpy restatements written here: integer dot products (fp64 products of integers below 2^53 are exact, so the
BLAS result cast to int64 is M8.astype(np.int64).T @ M8), the definitions of include/eagle_hip.h section 1b'' evaluated in the same
order, and a plain-loop greedy.  They share no code with the feature.  Every comparison is exact: integers, bits and bytes."""
import functools
import os

import numpy as np
import pytest

E2B_HEADER = 64


# ---- numpy restatements ----
def np_band_dots(M8, window, block=512):
    """d[i, o - 1] = sum over the individuals of g_i g_(i + o), int64 (L, window); 0 where i + o >= L."""
    G = np.asarray(M8, dtype=np.float64)
    n, L = G.shape
    d = np.zeros((L, window), dtype=np.int64)
    for r0 in range(0, L, block):
        r1, c1 = min(L, r0 + block), min(L, r0 + block + window)
        D = (G[:, r0:r1].T @ G[:, r0:c1]).astype(np.int64)               # exact: integers far below 2^53
        for o in range(1, window + 1):
            k = min(r1, L - o) - r0
            if k > 0:
                d[r0:r0 + k, o - 1] = D[np.arange(k), np.arange(k) + o]
    return d


def np_sv(M8):
    G = np.asarray(M8, dtype=np.int64)
    s, q = G.sum(axis=0), (G * G).sum(axis=0)
    return s, G.shape[0] * q - s * s


def np_mask(M8, window, t, d=None):
    """The definition: bit o - 1 of marker i iff v_i > 0, v_j > 0 and (double)c * (double)c > t * ((double)v_i * (double)v_j)."""
    n, L = M8.shape
    d = np_band_dots(M8, window) if d is None else d[:, :window]
    s, v = np_sv(M8)
    bits = np.zeros((L, (window + 63) // 64 * 64), dtype=np.uint8)
    for o in range(1, window + 1):
        k = L - o
        if k <= 0:
            break
        c = (n * d[:k, o - 1] - s[:k] * s[o:]).astype(np.float64)
        vi, vj = v[:k], v[o:]
        bits[:k, o - 1] = (vi > 0) & (vj > 0) & (c * c > np.float64(t) * (vi.astype(np.float64) * vj.astype(np.float64)))
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").astype(np.uint64)


def popcount(mask):
    return int(np.unpackbits(np.ascontiguousarray(mask).view(np.uint8)).sum())


def bit(mask, i, j):
    o = j - i
    return bool((int(mask[i, (o - 1) // 64]) >> ((o - 1) % 64)) & 1)


def np_pairs(mask, window):
    L = mask.shape[0]
    return [(i, i + o) for i in range(L) for o in range(1, window + 1) if i + o < L and bit(mask, i, i + o)]


def greedy(L, pairs, order):
    adj = [[] for _ in range(L)]
    for i, j in pairs:
        adj[i].append(j)
        adj[j].append(i)
    keep = np.zeros(L, dtype=bool)
    for i in order:
        keep[i] = not any(keep[j] for j in adj[i])
    return keep


# ---- panels ----
def write_table(path, digits):
    d = np.asarray(digits, dtype=np.uint8)
    buf = np.full((d.shape[0], 2 * d.shape[1]), ord(" "), dtype=np.uint8)
    buf[:, 0::2] = d + ord("0")
    buf[:, -1] = ord("\n")
    with open(path, "wb") as f:
        f.write(buf.tobytes())
    return str(path)


def ingest_text(tmp, name, M8):
    from eagleeverything_amd import r_api
    d = tmp / name
    d.mkdir()
    geno = r_api.ReadMarker(write_table(d / "table.txt", M8 + 1), type="text", AA=0, AB=1, BB=2, outdir=str(d))
    assert geno is not None and list(geno["dim_of_ascii_M"]) == list(M8.shape)
    return geno


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def assert_same_panel_files(a, b):
    """Both text files byte for byte; both sidecars: payload, and the header up to the text file's time stamp."""
    assert list(a["dim_of_ascii_M"]) == list(b["dim_of_ascii_M"])
    for key in ("asciifileM", "asciifileMt"):
        assert _read(a[key]) == _read(b[key]), key
        x, y = _read(a[key] + ".e2b"), _read(b[key] + ".e2b")
        assert len(x) == len(y) and x[E2B_HEADER:] == y[E2B_HEADER:] and x[:48] == y[:48], key


W = 50                     # the window of the planted panel
ANCHORS = (100, 127, 460, 480, 2000)   # a + W crosses row 128 (a tile edge), 127 | 128, and rows 510 .. 531 around row 512 (a window edge)


@functools.lru_cache(maxsize=None)
def planted_panel():
    """1,003 x 5,000 random with, for every anchor a: a + 1 a duplicate of a, a + W its complement (c < 0), a + W + 1 a duplicate
    again (distance W + 1 from a); 512 a duplicate of 511; three monomorphic markers; a duplicate pair as the last two markers."""
    from eagleeverything_amd import synth
    Mt8 = synth.genotypes_marker_major(1003, 5000, seed=1234)
    for a in ANCHORS:
        Mt8[a + 1], Mt8[a + W], Mt8[a + W + 1] = Mt8[a], -Mt8[a], Mt8[a]
    Mt8[512] = Mt8[511]
    Mt8[17], Mt8[2500], Mt8[3777] = -1, 0, 1
    Mt8[4999] = Mt8[4998]
    M8 = np.ascontiguousarray(Mt8.T)
    M8.setflags(write=False)
    return M8


@functools.lru_cache(maxsize=None)
def planted_dots():
    d = np_band_dots(planted_panel(), 256)
    d.setflags(write=False)
    return d


# ------------------------------------------------------------------------------------------------ 1. fixtures against numpy
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["genoDemo_150x4998", "synth_203x1531"])
def test_gpu_ld_window_equals_numpy(golden, tmp_path, case):
    from eagleeverything_amd import rcpp_api
    M8 = golden(case)["M8"]
    n, L = M8.shape
    assert n % 16 and L % 32 and L % 128
    d = np_band_dots(M8, 256)
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    windows = (1, 50, 64, 65, 256)
    # On the numpy masks alone, before the device is asked: neither an all-clear nor an all-set kernel can pass.  At r2 = 0.02 between
    # 0.5 % and 50 % of the bits of the bands checked are set (independent markers at n = 203: about 4 % at every window; the real panel:
    # 17 % at window 256, 21 % at 50 -- and 53.5 % of its ADJACENT pairs, window 1, which is why the share is taken over the five
    # bands together and every single band is only required to be neither empty nor full).
    set_bits = {w: popcount(np_mask(M8, w, 0.02, d)) for w in windows}
    bands = {w: sum(L - o for o in range(1, w + 1)) for w in windows}
    assert all(0 < set_bits[w] < bands[w] for w in windows), (set_bits, bands)
    assert 0.005 * sum(bands.values()) <= sum(set_bits.values()) <= 0.5 * sum(bands.values()), (set_bits, bands)
    for window in windows:
        for r2 in (0.02, 0.2):
            truth = np_mask(M8, window, r2, d)
            got, pairs = rcpp_api.ld_window(geno["asciifileMt"], (n, L), window, r2, return_pairs=True)
            assert got.dtype == np.uint64 and got.shape == (L, (window + 63) // 64)
            assert np.array_equal(got, truth), (window, r2, np.flatnonzero((got != truth).any(axis=1))[:10])
            assert pairs == popcount(truth)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 2. planted structure
@pytest.mark.gpu
def test_gpu_ld_planted_structure(tmp_path):
    from eagleeverything_amd import rcpp_api
    M8 = planted_panel()
    n, L = M8.shape
    d = planted_dots()
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    Mt = geno["asciifileMt"]
    truth = np_mask(M8, W, 0.2, d)
    got, pairs = rcpp_api.ld_window(Mt, (n, L), W, 0.2, return_pairs=True)
    assert np.array_equal(got, truth) and pairs == popcount(truth)
    for a in ANCHORS:
        assert bit(got, a, a + 1) and bit(got, a, a + W) and bit(got, a + 1, a + W + 1)      # duplicate, complement at W, duplicate at W
        assert not bit(got, a, a + 2)
    assert bit(got, 511, 512) and bit(got, 4998, 4999)
    assert not got[[17, 2500, 3777]].any()                                # a monomorphic marker is in LD with nothing ...
    for m in (17, 2500, 3777):
        assert not any(bit(got, m - o, m) for o in range(1, W + 1))       # ... from either side
    assert not got[4999].any() and int(got[4998, 0]) == 1                 # bits with i + o >= L are clear
    wide = rcpp_api.ld_window(Mt, (n, L), W + 1, 0.2)                     # the pair at distance W + 1 exists: one more marker of window
    assert np.array_equal(wide, np_mask(M8, W + 1, 0.2, d))               # sees it, and the window of W has no bit for it
    for a in ANCHORS:
        assert bit(wide, a, a + W + 1)
    assert popcount(wide) > pairs
    one = rcpp_api.ld_window(Mt, (n, L), W, 1.0)                          # strict '>': r^2 = 1 is not above 1
    assert not one.any() and not np_mask(M8, W, 1.0, d).any()
    t = 1.0 - 2.0 ** -50
    near = rcpp_api.ld_window(Mt, (n, L), W, t)
    assert np.array_equal(near, np_mask(M8, W, t, d))
    for a in ANCHORS:
        assert bit(near, a, a + 1) and bit(near, a, a + W)
    assert popcount(near) == 5 * len(ANCHORS) + 3                         # per anchor (a, a+1), (a, a+W), (a+1, a+W), (a+1, a+W+1) and
    zero = rcpp_api.ld_window(Mt, (n, L), W, 0.0)                         # (a+W, a+W+1); then (511, 512), (510, 512) and the last two
    assert np.array_equal(zero, np_mask(M8, W, 0.0, d))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 3. streamed equals resident
@pytest.mark.gpu
def test_gpu_ld_streamed_equals_resident(tmp_path, monkeypatch):
    from eagleeverything_amd import rcpp_api
    M8 = planted_panel()
    n, L = M8.shape
    d = planted_dots()
    loci = [0, 511, 512, 4999, 2500, 511, 100, 150]
    G = M8.astype(np.float64)
    dots_truth = (G.T @ G[:, loci]).astype(np.int64)
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    Mt = geno["asciifileMt"]
    resident = {w: rcpp_api.ld_window(Mt, (n, L), w, 0.2) for w in (W, 256)}
    for w in (W, 256):
        assert np.array_equal(resident[w], np_mask(M8, w, 0.2, d))
    dots = rcpp_api.ld_dots(Mt, (n, L), loci)
    assert dots.dtype == np.int32 and dots.shape == (L, len(loci)) and np.array_equal(dots, dots_truth)
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.001")              # 1 MB: the 5,120 x 1,024 image goes in row windows
    for sidecar in ("1", "0"):                                            # from the sidecar, then from the text
        monkeypatch.setenv("EAGLE_HIP_SIDECAR", sidecar)
        for w in (W, 256):
            got, pairs = rcpp_api.ld_window(Mt, (n, L), w, 0.2, return_pairs=True)
            assert np.array_equal(got, resident[w]), (sidecar, w, np.flatnonzero((got != resident[w]).any(axis=1))[:10])
            assert pairs == popcount(resident[w])
        assert np.array_equal(rcpp_api.ld_dots(Mt, (n, L), loci), dots)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 4. small edges
@pytest.mark.gpu
@pytest.mark.parametrize("L,window", [(100, 256), (1, 50), (33, 32), (33, 256)])
def test_gpu_ld_small_edges(tmp_path, L, window):
    from eagleeverything_amd import rcpp_api, synth
    n = 37
    Mt8 = synth.genotypes_marker_major(n, L, seed=L)
    if L > 40:
        Mt8[40] = Mt8[3]
        Mt8[L - 1] = -Mt8[0]
    M8 = np.ascontiguousarray(Mt8.T)
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    for r2 in (0.02, 0.3):
        truth = np_mask(M8, window, r2)
        got, pairs = rcpp_api.ld_window(geno["asciifileMt"], (n, L), window, r2, return_pairs=True)
        assert got.shape == (L, (window + 63) // 64) and np.array_equal(got, truth) and pairs == popcount(truth)
    if L > 40:
        assert bit(got, 3, 40) and bit(got, 0, L - 1)
    G = M8.astype(np.int64)
    assert np.array_equal(rcpp_api.ld_dots(geno["asciifileMt"], (n, L), [L - 1, 0]), (G.T @ G)[:, [L - 1, 0]])
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 5. n d beyond int32
@pytest.mark.gpu
def test_gpu_ld_int64_products(tmp_path):
    from eagleeverything_amd import rcpp_api, synth
    n, L = 46400, 300
    Mt8 = synth.genotypes_marker_major(n, L, seed=46)
    common = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int8)      # half +1, half -1: d(0, 7) = n, n d = 2.15e9 > 2^31
    np.random.default_rng(46).shuffle(common)
    Mt8[0] = common
    Mt8[7] = common
    Mt8[9] = -common
    M8 = np.ascontiguousarray(Mt8.T)
    assert n * int(M8[:, 0].astype(np.int64) @ M8[:, 7]) > 2 ** 31
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    d = np_band_dots(M8, 50)
    for r2 in (0.0001, 0.2):
        truth = np_mask(M8, 50, r2, d)
        got = rcpp_api.ld_window(geno["asciifileMt"], (n, L), 50, r2)
        assert np.array_equal(got, truth)
    assert bit(got, 0, 7) and bit(got, 0, 9) and bit(got, 7, 9) and popcount(got) == 3
    loci = [0, 7, 9, 299]
    G = M8.astype(np.float64)
    dots = rcpp_api.ld_dots(geno["asciifileMt"], (n, L), loci)
    assert np.array_equal(dots, (G.T @ G[:, loci]).astype(np.int64)) and dots[0, 1] == n and dots[0, 2] == -n
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 6. a VIEW alias
@pytest.mark.gpu
def test_gpu_ld_on_view_alias(golden, tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    na = np.array([1, 2, 57, 130, 203])                                   # 1-based, as R hands them over
    kept = np.setdiff1d(np.arange(n), na - 1)
    dims = r_api.ReshapeM(geno["asciifileM"], geno["asciifileMt"], na, (n, L), view=True)
    assert dims[0] == n - 5
    sub = np.ascontiguousarray(M8[kept])
    truth = np_mask(sub, 70, 0.05)
    assert not np.array_equal(truth, np_mask(M8, 70, 0.05))               # the five individuals matter
    got = rcpp_api.ld_window(geno["asciifileMt"] + "tmp", (n - 5, L), 70, 0.05)
    assert np.array_equal(got, truth)
    G = sub.astype(np.int64)
    assert np.array_equal(rcpp_api.ld_dots(geno["asciifileMt"] + "tmp", (n - 5, L), [5, 1530]), (G.T @ G)[:, [5, 1530]])
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 7. ld_dots / LDofLoci
@pytest.mark.gpu
def test_gpu_ld_dots_and_ldofloci(golden, tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    G = M8.astype(np.int64)
    full = G.T @ G
    s, v = np_sv(M8)
    assert (v > 0).all()
    rng = np.random.default_rng(11)
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    stats = r_api.MarkerStats(geno)
    for k in (1, 20, 64, 70):                                             # 70: LDofLoci makes two passes
        loci = rng.integers(0, L, k)
        loci[0] = L - 1                                                   # in the last, partial tile of 128 markers
        if k > 2:
            loci[-1] = loci[1]                                            # a repeated locus
        if k <= 64:
            dots = rcpp_api.ld_dots(geno["asciifileMt"], (n, L), loci)
            assert dots.dtype == np.int32 and dots.shape == (L, k) and np.array_equal(dots, full[:, loci])
        out = r_api.LDofLoci(geno, loci, stats=stats)
        assert np.array_equal(out["loci"], loci) and np.array_equal(out["dots"], full[:, loci]) and out["r2"].shape == (L, k)
        c = (n * full[:, loci] - s[:, None] * s[loci][None, :]).astype(np.float64)
        assert np.array_equal(out["r2"], c * c / (v.astype(np.float64)[:, None] * v[loci].astype(np.float64)[None, :]))
        assert all(out["r2"][j, col] == 1.0 for col, j in enumerate(loci))
    assert np.array_equal(r_api.LDofLoci(geno, [3])["r2"], r_api.LDofLoci(geno, [3], stats=stats)["r2"])
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 8. LDPrune end to end
def ld_panel(n, L, seed):
    """Runs of correlated markers: every marker is, with probability 0.6, its predecessor with 4 % of the genotypes redrawn."""
    from eagleeverything_amd import synth
    Mt8 = synth.genotypes_marker_major(n, L, seed=seed)
    rng = np.random.default_rng(seed)
    for j in range(1, L):
        if rng.random() < 0.6:
            fresh = rng.random(n) < 0.04
            Mt8[j] = np.where(fresh, Mt8[j], Mt8[j - 1])
    return Mt8


@pytest.mark.gpu
def test_gpu_ldprune_end_to_end(tmp_path):
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    n, L, window, r2 = 301, 3000, 50, 0.2
    Mt8 = ld_panel(n, L, 21)
    M8 = np.ascontiguousarray(Mt8.T)
    y, qtl = synth.trait(Mt8, nqtl=3, beta=1.0, seed=5)
    chrom = ["1" if j < 1700 else "2" for j in range(L)]
    pos = (np.cumsum(np.random.default_rng(2).integers(200, 3000, L)) + 1).tolist()
    bim = {"SNP": ["snp%d" % (j + 1) for j in range(L)], "Chr": chrom, "Pos": pos}
    truth = np_mask(M8, window, r2)
    pairs = np_pairs(truth, window)
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "src", M8)
    fM, fMt = geno["asciifileM"], geno["asciifileMt"]

    def reference(name, keep_idx, src=geno):
        d = tmp_path / name
        d.mkdir()
        dims = rcpp_api.filter_markers(src["asciifileM"], src["asciifileMt"], src["dim_of_ascii_M"], keep_idx, str(d / "M.ascii"), str(d / "Mt.ascii"))
        return {"asciifileM": str(d / "M.ascii"), "asciifileMt": str(d / "Mt.ascii"), "dim_of_ascii_M": dims}

    def same_resident_images(a, b, k):
        dims = (n, k)
        assert np.array_equal(rcpp_api.marker_counts(a["asciifileMt"], dims), rcpp_api.marker_counts(b["asciifileMt"], dims))
        loci = [0, k // 2, k - 1]
        assert np.array_equal(rcpp_api.ld_dots(a["asciifileMt"], dims, loci), rcpp_api.ld_dots(b["asciifileMt"], dims, loci))
        assert np.array_equal(rcpp_api.calculateMMt_rcpp(a["asciifileM"], 8.0, 4, np.nan, dims), rcpp_api.calculateMMt_rcpp(b["asciifileM"], 8.0, 4, np.nan, dims))

    # a. position order, no map
    keep = np.flatnonzero(greedy(L, pairs, range(L)))
    assert 0.2 * L < keep.size < 0.8 * L
    msgs = []
    pruned = r_api.LDPrune(geno, window=window, r2=r2, message=msgs.append)
    assert pruned["asciifileM"] == os.path.join(os.path.dirname(fM), "ld", "M.ascii")
    assert pruned["marker_index"].dtype == np.int64 and np.array_equal(pruned["marker_index"], keep)
    assert list(pruned["dim_of_ascii_M"]) == [n, keep.size] and any("%d of %d markers kept" % (keep.size, L) in m for m in msgs)
    ref = reference("ref_a", keep)
    assert_same_panel_files(pruned, ref)
    same_resident_images(pruned, ref, keep.size)
    # a pruned panel pruned again at the same settings loses nothing more than the greedy says (its own pairs are all gone)
    again = r_api.LDPrune(pruned, window=window, r2=r2, outdir=str(tmp_path / "again"))
    sub_pairs = np_pairs(np_mask(M8[:, keep], window, r2), window)
    keep2 = np.flatnonzero(greedy(keep.size, sub_pairs, range(keep.size)))
    assert np.array_equal(again["marker_index"], keep[keep2])

    # b. prefer="maf" with a map and kb=
    kb = 20
    cut = [(i, j) for i, j in pairs if chrom[i] == chrom[j] and abs(pos[i] - pos[j]) <= 1000 * kb]
    assert 0 < len(cut) < len(pairs) and any(chrom[i] != chrom[j] for i, j in pairs)
    G = M8.astype(np.int64)
    n0, n1, n2 = (G == -1).sum(0), (G == 0).sum(0), (G == 1).sum(0)
    maf = np.minimum(2 * n2 + n1, 2 * n0 + n1) / (2.0 * n)
    order = sorted(range(L), key=lambda i: (-maf[i], i))
    keep_b = np.flatnonzero(greedy(L, cut, order))
    assert not np.array_equal(keep_b, keep)
    pruned_b = r_api.LDPrune(geno, window=window, r2=r2, prefer="maf", map=bim, kb=kb, outdir=str(tmp_path / "out_b"))
    assert np.array_equal(pruned_b["marker_index"], keep_b)
    assert_same_panel_files(pruned_b, reference("ref_b", keep_b))

    # c. an already filtered panel: marker_index composes, and the source's map is taken through it
    flt = r_api.FilterMarkers(geno, maf=0.3, outdir=str(tmp_path / "qc"))
    f_idx = np.flatnonzero(maf >= 0.3)
    assert np.array_equal(flt["marker_index"], f_idx) and 100 < f_idx.size < L
    f_pairs = [(i, j) for i, j in np_pairs(np_mask(M8[:, f_idx], window, r2), window) if chrom[f_idx[i]] == chrom[f_idx[j]]]
    keep_c = np.flatnonzero(greedy(f_idx.size, f_pairs, range(f_idx.size)))
    pruned_c = r_api.LDPrune(flt, window=window, r2=r2, map=bim, outdir=str(tmp_path / "out_c"))
    assert np.array_equal(pruned_c["marker_index"], f_idx[keep_c])
    assert_same_panel_files(pruned_c, reference("ref_c", keep_c, src=flt))

    # d. AM() on the pruned panel, and the markers that tag its picks in the source panel
    X = np.ones((n, 1))
    res = am.AM(y, X, pruned, maxit=4)
    assert len(res["selected_loci"]) >= 1
    picked = pruned["marker_index"][np.array(res["selected_loci"], dtype=np.int64) - 1]
    src_obj = dict(res, selected_loci=[int(j) + 1 for j in picked])       # the picks under their source indices
    tags = am.tag_markers(src_obj, geno, r2=0.8, map=bim)
    s, v = np_sv(M8)
    full = G.T @ G
    assert [t["locus"] for t in tags] == src_obj["selected_loci"]
    for t, j in zip(tags, picked):
        c = (n * full[:, j] - s * s[j]).astype(np.float64)
        exp = np.flatnonzero(c * c / (v.astype(np.float64) * float(v[j])) >= 0.8)
        assert j in exp and np.array_equal(t["markers"], exp + 1) and t["names"] == [bim["SNP"][i] for i in exp]
        on = [pos[i] for i in exp if chrom[i] == chrom[j]]
        assert t["chrom"] == chrom[j] and t["span"] == (min(on), max(on))
    tags_pruned = am.tag_markers(res, pruned, r2=0.8)                     # in the pruned panel a pick still tags itself
    assert all(t["locus"] in t["markers"].tolist() for t in tags_pruned)
    rcpp_api.drop_cache()
