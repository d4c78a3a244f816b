"""Sample QC on the GPU: eagle_sample_counts / eagle_bed_sample_counts / eagle_sample_ibs / eagle_hwe_exact (k_marker_counts on the
individual-major image, k_bed_sample_counts, two fp4 SYRKs + k_f4_abs + k_ibs_finish, k_hwe_exact) and the r_api interface on top
(SampleStats, Relatedness, related_drop, HWE, FilterMarkers(hwe=)).

Expected values are numpy or plain-Python restatements written here from the definitions of include/eagle_hip.h section 1b''': counts
by comparison, the two Gram products in float64 (integers far below 2^53 are exact), the exact test as a scalar loop in the header's
order and, independently, in fractions.Fraction.  They share no code with the feature.  Every integer comparison is array_equal, the
exact test is compared bit for bit."""
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

E2B_HEADER = 64


# ---- restatements ----
def np_sample_counts(M8):
    """(n, 3) counts of -1 / 0 / +1 per individual of an n x L int8 matrix."""
    return np.stack([np.sum(M8 == v, axis=1) for v in (-1, 0, 1)], axis=1).astype(np.int32)


def np_ibs(M8):
    """ibs0, hethet (int64, n x n) of an n x L matrix of -1 / 0 / +1: from the float64 Grams, or pair by pair for a small panel."""
    G = np.asarray(M8, dtype=np.float64)
    n, L = G.shape
    if n <= 40:
        ibs0, hethet = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
        for i in range(n):
            for j in range(n):
                ibs0[i, j] = np.sum((M8[i] == -1) & (M8[j] == 1)) + np.sum((M8[i] == 1) & (M8[j] == -1))
                hethet[i, j] = np.sum((M8[i] == 0) & (M8[j] == 0))
        return ibs0, hethet
    D = (G @ G.T).astype(np.int64)
    Q = ((G * G) @ (G * G).T).astype(np.int64)
    q = np.diagonal(Q)
    assert np.all((Q - D) % 2 == 0)
    return (Q - D) // 2, L - q[:, None] - q[None, :] + Q


def np_king(ibs0, hethet):
    h = np.diagonal(hethet).astype(np.int64)
    num = (hethet.astype(np.int64) - 2 * ibs0.astype(np.int64)).astype(np.float64)
    den = (h[:, None] + h[None, :]).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.where(den == 0, np.nan, num / den)


def py_hwe(n_aa, n_ab, n_bb):
    """The exact test in the order the header fixes: mid, the lower leg, the upper leg; one rounding per product, quotient, sum."""
    N = n_aa + n_ab + n_bb
    if N == 0:
        return 1.0
    r = 2 * min(n_aa, n_bb) + n_ab
    mid = r * (2 * N - r) // (2 * N)
    if (mid ^ r) & 1:
        mid += 1
    hr0 = (r - mid) // 2
    hc0 = N - mid - hr0

    def walk(cut):
        s = 1.0 if (cut is None or 1.0 <= cut) else 0.0
        pobs = 1.0
        p, a, b, h = 1.0, hr0, hc0, mid
        while h >= 2:
            p = (p * float(h * (h - 1))) / float(4 * (a + 1) * (b + 1))
            a, b, h = a + 1, b + 1, h - 2
            if h == n_ab:
                pobs = p
            if cut is None or p <= cut:
                s = s + p
        p, a, b, h = 1.0, hr0, hc0, mid
        while h <= r - 2:
            p = (p * float(4 * a * b)) / float((h + 2) * (h + 1))
            a, b, h = a - 1, b - 1, h + 2
            if h == n_ab:
                pobs = p
            if cut is None or p <= cut:
                s = s + p
        return s, pobs
    total, pobs = walk(None)
    return min(1.0, walk(pobs)[0] / total)


def frac_hwe(n_aa, n_ab, n_bb):
    """The same test in exact rational arithmetic, walked upwards from the smallest heterozygote count."""
    N = n_aa + n_ab + n_bb
    if N == 0:
        return Fraction(1)
    r = 2 * min(n_aa, n_bb) + n_ab
    h = r % 2
    P = {h: Fraction(1)}
    while h <= r - 2:
        hr = (r - h) // 2
        P[h + 2] = P[h] * Fraction(4 * hr * (N - h - hr), (h + 2) * (h + 1))
        h += 2
    return min(Fraction(1), sum(v for v in P.values() if v <= P[n_ab]) / sum(P.values()))


def py_hwe_rows(counts):
    """py_hwe of every row of an (L, >= 3) integer array (each distinct row evaluated once)."""
    c = np.asarray(counts)[:, :3].astype(np.int64)
    uniq, inv = np.unique(c, axis=0, return_inverse=True)
    return np.array([py_hwe(*row) for row in uniq.tolist()], dtype=np.float64)[np.asarray(inv).ravel()]


def decode_bed_codes(path, n, L):
    raw = np.fromfile(path, dtype=np.uint8)
    rb = (n + 3) // 4
    assert raw.size == 3 + L * rb and tuple(raw[:3]) == (0x6c, 0x1b, 0x01)
    rows = raw[3:].reshape(L, rb)
    return np.stack([(rows >> (2 * q)) & 3 for q in range(4)], axis=2).reshape(L, 4 * rb)[:, :n]


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


DUPLICATES = ((5, 900), (0, 1002))
FAMILIES = ((10, 700, (400, 401)), (384, 767, (383,)))      # (parent, parent, children): 383 | 384 and 767 | 768 are tile edges
PLANTED = sorted([(5, 900), (0, 1002), (10, 400), (400, 700), (10, 401), (401, 700), (400, 401), (383, 384), (383, 767)])


@functools.lru_cache(maxsize=None)
def planted_panel():
    """1,003 x 5,000 random (n crosses the 256, 384 and 768 tile edges of the SYRK, L is no multiple of 256) with two duplicated
    individuals and three children, each parent passing one allele per marker.  -> (M8 n x L, ibs0, hethet, phi), read-only."""
    from eagleeverything_amd import synth
    M8 = np.ascontiguousarray(synth.genotypes_marker_major(1003, 5000, seed=1234).T)
    rng = np.random.default_rng(77)
    for a, b in DUPLICATES:
        M8[b] = M8[a]
    for pa, pb, children in FAMILIES:
        for c in children:
            ga = np.where(M8[pa] == 0, rng.integers(0, 2, M8.shape[1]), (M8[pa] + 1) // 2)    # the allele (0 / 1) each parent passes
            gb = np.where(M8[pb] == 0, rng.integers(0, 2, M8.shape[1]), (M8[pb] + 1) // 2)
            M8[c] = (ga + gb - 1).astype(np.int8)
    ibs0, hethet = np_ibs(M8)
    phi = np_king(ibs0, hethet)
    for a in (M8, ibs0, hethet, phi):
        a.setflags(write=False)
    return M8, ibs0, hethet, phi


def upper_pairs(mask):
    i, j = np.nonzero(np.triu(mask, k=1))
    return sorted(zip(i.tolist(), j.tolist()))


# ------------------------------------------------------------------------------------------------ 1. fixtures against numpy
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["genoDemo_150x4998", "synth_203x1531"])
def test_gpu_sample_counts_and_ibs_on_fixtures(golden, tmp_path, case):
    from eagleeverything_amd import r_api, rcpp_api
    M8 = golden(case)["M8"]
    n, L = M8.shape
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    counts = rcpp_api.sample_counts(geno["asciifileM"], (n, L))
    assert counts.dtype == np.int32 and counts.shape == (n, 3) and np.array_equal(counts, np_sample_counts(M8))
    assert np.array_equal(counts.sum(axis=1), np.full(n, L))
    ibs0_t, hethet_t = np_ibs(M8)
    i, j = 3, 77                                                       # the Gram restatement against the definition on one pair
    assert ibs0_t[i, j] == ((M8[i] == -1) & (M8[j] == 1)).sum() + ((M8[i] == 1) & (M8[j] == -1)).sum()
    assert hethet_t[i, j] == ((M8[i] == 0) & (M8[j] == 0)).sum()
    ibs0, hethet = rcpp_api.sample_ibs(geno["asciifileM"], (n, L))
    assert ibs0.dtype == np.int32 and ibs0.shape == (n, n) and hethet.dtype == np.int32 and hethet.shape == (n, n)
    assert np.array_equal(ibs0, ibs0_t) and np.array_equal(hethet, hethet_t)
    assert np.array_equal(np.diagonal(ibs0), np.zeros(n)) and np.array_equal(np.diagonal(hethet), counts[:, 1])
    phi = r_api.king_from_counts(ibs0, hethet)
    assert np.array_equal(phi, np_king(ibs0_t, hethet_t), equal_nan=True) and np.array_equal(np.diagonal(phi), np.full(n, 0.5))
    stats = r_api.SampleStats(geno)
    assert np.array_equal(stats["n1"], counts[:, 1]) and np.array_equal(stats["hom_count"], counts[:, 0] + counts[:, 2])
    assert np.array_equal(stats["het_rate"], counts[:, 1] / float(L)) and "call_rate" not in stats and np.isfinite(stats["F"]).all()
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 2. planted relatives across tile edges
@pytest.mark.gpu
def test_gpu_relatedness_finds_planted_relatives(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    M8, ibs0_t, hethet_t, phi_t = planted_panel()
    n, L = M8.shape
    # the numpy truth first: the planted pairs are exactly those above the second-degree cut, the duplicates those above 0.354
    assert upper_pairs(phi_t > 0.0884) == PLANTED and upper_pairs(phi_t > 0.177) == PLANTED
    assert upper_pairs(phi_t > 0.354) == sorted(DUPLICATES) and all(phi_t[a, b] == 0.5 for a, b in DUPLICATES)
    for pa, pb, children in FAMILIES:
        for c in children:
            assert ibs0_t[pa, c] == 0 and ibs0_t[pb, c] == 0
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    rel = r_api.Relatedness(geno)
    assert np.array_equal(rel["ibs0"], ibs0_t) and np.array_equal(rel["hethet"], hethet_t)
    assert np.array_equal(rel["kinship"], phi_t, equal_nan=True)
    assert rel["pairs"].dtype == np.int64 and rel["pairs"].tolist() == [list(p) for p in PLANTED]
    assert np.array_equal(rel["phi"], np.array([phi_t[a, b] for a, b in PLANTED]))
    assert sorted(rel["degree"]) == ["duplicate"] * 2 + ["first"] * 7
    assert [d for p, d in zip(PLANTED, rel["degree"]) if p in DUPLICATES] == ["duplicate", "duplicate"]
    for pa, pb, children in FAMILIES:
        for c in children:
            assert rel["ibs0"][pa, c] == 0 and rel["ibs0"][c, pb] == 0
    drop = r_api.related_drop(rel["pairs"], n)
    gone = set((drop - 1).tolist())
    assert drop.dtype == np.int64 and np.all(np.diff(drop) > 0) and all(a in gone or b in gone for a, b in PLANTED)
    assert gone == {401, 400, 383, 900, 1002}                          # the most pairs first, ties to the higher index
    # the kept individuals, as a VIEW: nothing related remains
    kept = np.setdiff1d(np.arange(n), drop - 1)
    from eagleeverything_amd import am
    sub = am.reshape_geno(geno, drop, view=True)
    assert list(sub["dim_of_ascii_M"])[0] == n - 5
    rel2 = r_api.Relatedness(sub)
    assert rel2["pairs"].shape == (0, 2) and np.array_equal(rel2["ibs0"], ibs0_t[np.ix_(kept, kept)])
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 3. streamed equals resident
@pytest.mark.gpu
def test_gpu_sample_ibs_streamed_equals_resident(tmp_path, monkeypatch):
    from eagleeverything_amd import rcpp_api
    M8, ibs0_t, hethet_t, _ = planted_panel()
    n, L = M8.shape
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    res = rcpp_api.sample_ibs(geno["asciifileM"], (n, L))
    cnt = rcpp_api.sample_counts(geno["asciifileM"], (n, L))
    assert np.array_equal(res[0], ibs0_t) and np.array_equal(res[1], hethet_t) and np.array_equal(cnt, np_sample_counts(M8))
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.001")          # windows of 256 markers, from the sidecar
    assert os.path.exists(geno["asciifileM"] + ".e2b")
    got = rcpp_api.sample_ibs(geno["asciifileM"], (n, L))
    assert got[0].tobytes() == res[0].tobytes() and got[1].tobytes() == res[1].tobytes()
    assert np.array_equal(rcpp_api.sample_counts(geno["asciifileM"], (n, L)), cnt)
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")                      # the same windows from the text
    got = rcpp_api.sample_ibs(geno["asciifileM"], (n, L))
    assert got[0].tobytes() == res[0].tobytes() and got[1].tobytes() == res[1].tobytes()
    assert np.array_equal(rcpp_api.sample_counts(geno["asciifileM"], (n, L)), cnt)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 4. the cached image is untouched
@pytest.mark.gpu
def test_gpu_sample_ibs_leaves_the_cached_operand_alone(golden, tmp_path):
    from eagleeverything_amd import rcpp_api
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    truth = (M8.astype(np.float64) @ M8.astype(np.float64).T)
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    before = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L))     # makes the cached fp4 image
    assert np.array_equal(before, truth)
    ibs = rcpp_api.sample_ibs(geno["asciifileM"], (n, L))
    after = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L))
    assert after.tobytes() == before.tobytes()
    # and the other way round: the image sample_ibs makes on a fresh file is the one calculateMMt would have made
    rcpp_api.drop_cache()
    ibs2 = rcpp_api.sample_ibs(geno["asciifileM"], (n, L))
    assert np.array_equal(ibs2[0], ibs[0]) and np.array_equal(ibs2[1], ibs[1])
    assert rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L)).tobytes() == before.tobytes()
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 5. small edges
@pytest.mark.gpu
@pytest.mark.parametrize("n,L", [(1, 1), (2, 33), (37, 33), (37, 300)])
def test_gpu_sample_ibs_small_edges(tmp_path, n, L):
    from eagleeverything_amd import r_api, rcpp_api, synth
    rng = np.random.default_rng(100 * n + L)
    M8 = rng.integers(-1, 2, size=(n, L)).astype(np.int8)
    M8[0] = rng.choice(np.array([-1, 1], dtype=np.int8), size=L)       # all homozygous
    if n > 1:
        M8[1] = rng.choice(np.array([-1, 1], dtype=np.int8), size=L)   # a second one: h_0 + h_1 = 0
    if n > 2:
        M8[2, 0] = 0                                                   # at least one heterozygous genotype
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), np.ascontiguousarray(M8.T))
    ibs0_t, hethet_t = np_ibs(M8)
    ibs0, hethet = rcpp_api.sample_ibs(geno["asciifileM"], (n, L))
    assert np.array_equal(ibs0, ibs0_t) and np.array_equal(hethet, hethet_t)
    assert np.array_equal(rcpp_api.sample_counts(geno["asciifileM"], (n, L)), np_sample_counts(M8))
    rel = r_api.Relatedness(geno, threshold=-10.0)                     # every pair with a kinship is reported
    phi_t = np_king(ibs0_t, hethet_t)
    assert np.array_equal(rel["kinship"], phi_t, equal_nan=True) and np.isnan(rel["kinship"][0, 0])
    want = [list(p) for p in upper_pairs(~np.isnan(phi_t))]
    assert rel["pairs"].tolist() == want and len(rel["degree"]) == len(want)
    if n > 1:
        assert np.isnan(rel["kinship"][0, 1]) and [0, 1] not in rel["pairs"].tolist()
    if n > 2:
        assert [0, 2] in rel["pairs"].tolist()
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 6. .bed sample counts
@functools.lru_cache(maxsize=None)
def bed_panel(n):
    from eagleeverything_amd import synth
    L = 1500                                                           # two blocks of 1,020 rows, flushes of 255 inside them
    Mt8 = synth.genotypes_marker_major(n, L, seed=900 + n)
    missing = np.random.default_rng(n).random((L, n)) < 0.03
    missing[:, n - 1] |= np.arange(L) % 3 == 0                         # the last individual (the last byte's last used field)
    return Mt8, missing


@pytest.mark.gpu
@pytest.mark.parametrize("n", [150, 203, 1003])
def test_gpu_bed_sample_counts(tmp_path, n):
    from eagleeverything_amd import r_api, rcpp_api, synth
    assert n % 4 != 0
    Mt8, missing = bed_panel(n)
    L = Mt8.shape[0]
    bed = synth.write_bed(str(tmp_path / "panel"), Mt8, missing=missing)
    codes = decode_bed_codes(bed, n, L)                                # L x n
    truth = np.stack([np.sum(codes == v, axis=0) for v in (0, 2, 3, 1)], axis=1).astype(np.int32)
    assert np.array_equal(truth[:, 3], missing.sum(axis=0)) and truth[:, 3].min() > 0
    got = rcpp_api.bed_sample_counts(bed, (n, L))
    assert got.dtype == np.int32 and got.shape == (n, 4) and np.array_equal(got, truth)
    assert np.array_equal(got.sum(axis=1), np.full(n, L))
    assert np.array_equal(got.sum(axis=0), rcpp_api.bed_marker_counts(bed, (n, L)).sum(axis=0))
    rb = (n + 3) // 4
    small = rcpp_api.bed_sample_counts(bed, (n, L), max_memory_in_Gbytes=4 * 100 * rb / 1e9)   # windows of 100 markers
    assert np.array_equal(small, truth)
    stats = r_api.SampleStats({"dim_of_ascii_M": [n, L]}, bed=bed)
    assert np.array_equal(stats["n_missing"], truth[:, 3]) and np.array_equal(stats["call_rate"], (L - truth[:, 3]) / float(L))
    assert np.array_equal(stats["het_rate"], truth[:, 1] / (L - truth[:, 3]).astype(np.float64))


# ------------------------------------------------------------------------------------------------ 7. the exact test
@pytest.mark.gpu
def test_gpu_hwe_exact_bits_and_fractions(golden, tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    sets = []
    for case in ("genoDemo_150x4998", "synth_203x1531"):
        M8 = golden(case)["M8"]
        sets.append(np.stack([np.sum(M8 == v, axis=0) for v in (-1, 0, 1)], axis=1).astype(np.int32))
    for n in (150, 203):
        Mt8, missing = bed_panel(n)
        G = np.where(missing, 9, Mt8)
        sets.append(np.stack([np.sum(G == v, axis=1) for v in (-1, 0, 1, 9)], axis=1).astype(np.int32))    # stride 4
    for counts in sets:
        truth = py_hwe_rows(counts)
        assert (truth < 0.05).any() and (truth >= 0.05).any() and np.all((truth > 0) & (truth <= 1))       # on the restatement alone
        got = rcpp_api.hwe_exact(counts)
        assert got.dtype == np.float64 and got.shape == (counts.shape[0],)
        assert got.tobytes() == truth.tobytes()
        uniq, first = np.unique(counts[:, :3], axis=0, return_index=True)
        assert uniq.sum(axis=1).max() <= 300
        for row, k in zip(uniq.tolist(), first.tolist()):
            exact = frac_hwe(*row)
            assert abs(Fraction(float(got[k])) - exact) <= Fraction(1, 10 ** 12) * exact, (row, got[k], float(exact))
    hand = np.array([[0, 0, 0], [120, 0, 0], [0, 0, 77], [50, 0, 50], [25, 50, 25], [1, 0, 0]], dtype=np.int32)
    p = rcpp_api.hwe_exact(hand)
    assert p[0] == 1.0 and p[1] == 1.0 and p[2] == 1.0 and 0 < p[3] < 1e-20 and p[4] == 1.0 and p[5] == 1.0
    assert p.tobytes() == py_hwe_rows(hand).tobytes()
    assert np.array_equal(r_api.HWE({"n0": hand[:, 0], "n1": hand[:, 1], "n2": hand[:, 2]}), p) and np.array_equal(r_api.HWE(hand), p)
    with pytest.raises(ValueError):
        rcpp_api.hwe_exact(hand[:, :2])


# ------------------------------------------------------------------------------------------------ 8. end to end
@pytest.mark.gpu
def test_gpu_filter_markers_hwe(golden, tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    M8 = golden("genoDemo_150x4998")["M8"]
    n, L = M8.shape
    counts = np.stack([np.sum(M8 == v, axis=0) for v in (-1, 0, 1)], axis=1)
    p = py_hwe_rows(counts)
    idx = np.flatnonzero(~(p < 1e-3))
    assert 0 < idx.size < L
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "src", M8)
    stats = r_api.MarkerStats(geno)
    assert "hwe_p" not in stats                                        # the default output is unchanged
    stats = r_api.MarkerStats(geno, hwe=True)
    assert stats["hwe_p"].tobytes() == p.tobytes()
    assert np.array_equal(np.flatnonzero(r_api.marker_keep_mask(stats, hwe=1e-3)), idx)
    flt = r_api.FilterMarkers(geno, hwe=1e-3, outdir=str(tmp_path / "flt"))
    assert np.array_equal(flt["marker_index"], idx) and list(flt["dim_of_ascii_M"]) == [n, idx.size]
    (tmp_path / "ref").mkdir()
    ref = {"asciifileM": str(tmp_path / "ref" / "M.ascii"), "asciifileMt": str(tmp_path / "ref" / "Mt.ascii")}
    ref["dim_of_ascii_M"] = rcpp_api.filter_markers(geno["asciifileM"], geno["asciifileMt"], (n, L), idx, ref["asciifileM"], ref["asciifileMt"])
    assert_same_panel_files(flt, ref)
    both = r_api.FilterMarkers(geno, hwe=1e-3, maf=0.05, stats=r_api.MarkerStats(geno), outdir=str(tmp_path / "both"))   # p-values added
    maf = np.minimum(2 * counts[:, 2] + counts[:, 1], 2 * counts[:, 0] + counts[:, 1]) / (2.0 * n)
    assert np.array_equal(both["marker_index"], np.flatnonzero(~(p < 1e-3) & (maf >= 0.05)))
    rcpp_api.drop_cache()


@pytest.mark.gpu
def test_gpu_sample_stats_to_am_on_the_kept_individuals(golden, tmp_path):
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    M8 = golden("synth_203x1531")["M8"].copy()
    n, L = M8.shape
    rng = np.random.default_rng(11)
    M8[7, rng.random(L) < 0.6] = 0                                     # a contaminated sample: far too heterozygous
    M8[150, M8[150] == 0] = 1                                          # an inbred one: no heterozygous genotype
    y, qtl = synth.trait(np.ascontiguousarray(M8.T), nqtl=3, beta=1.5, seed=5)
    X = np.ones((n, 1))
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "src", M8)
    stats = r_api.SampleStats(geno)
    het = np.sum(M8 == 0, axis=1) / float(L)
    assert np.array_equal(stats["het_rate"], het) and stats["F"][150] == 1.0 and stats["F"][7] < -0.5
    keep = r_api.sample_keep_mask(stats, het_sd=3.0)
    want = np.abs(het - het.mean()) <= 3.0 * het.std(ddof=1)
    assert np.array_equal(keep, want) and sorted(np.flatnonzero(~keep).tolist()) == [7, 150]
    drop = r_api.sample_drop_index(keep)
    assert drop.tolist() == [8, 151]
    sub = am.reshape_geno(geno, drop, view=True)
    assert list(sub["dim_of_ascii_M"]) == [n - 2, L]
    res = am.AM(y[keep], X[keep], sub, maxit=3)
    rcpp_api.drop_cache()
    ref = am.AM(y[keep], X[keep], ingest_text(tmp_path, "ref", M8[keep]), maxit=3)
    assert res["selected_loci"] == ref["selected_loci"] and len(res["selected_loci"]) >= 1
    rcpp_api.drop_cache()
