"""Pairwise-complete IBS counts on the GPU: eagle_bed_sample_ibs (k_bed_pack_fp4, four fp4 SYRKs, k_bed_ibs_finish) and
eagle_knn_rows_dist (k_knn_rows_dist), with Relatedness(bed=) and ImputeBed(pairwise=True) on top.

The device's five matrices are compared with r_api.bed_ibs_host and the neighbour table with r_api.knn_rows_host -- the numpy
restatements that tests/test_bed_ibs_host.py and tests/test_impute_host.py pin to plain loops of the definitions.  Everything is an
integer or a byte: every comparison is ==, and phi of a duplicate pair is 0.5 exactly."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEAD = b"\x6c\x1b\x01"
NO_OVERLAP = 0xFFFFFFFE
NAMES = ("ncalled", "ibs0", "hethet", "hetsum", "dist")


@functools.lru_cache(maxsize=None)
def make_panel(n, L, seed, rate=0.15, lost=False):
    """(Mt8, missing) of a random panel with the planted cases the shape allows: individuals 0 and 1 are one genotype vector under
    two masks, marker 0 has no call, marker 1 no missing code; lost: the last individual has no call at all (which marker 1 then
    shares)."""
    rng = np.random.default_rng(seed)
    Mt8 = rng.integers(-1, 2, size=(L, n)).astype(np.int8)
    miss = rng.random((L, n)) < rate
    if n >= 2:
        Mt8[:, 1] = Mt8[:, 0]
    if L >= 2:
        miss[0, :] = True
        miss[1, :] = False
    if lost:
        miss[:, n - 1] = True
    Mt8.setflags(write=False)
    miss.setflags(write=False)
    return Mt8, miss


def codes_of(Mt8, miss):
    codes = np.array([0, 2, 3], dtype=np.uint8)[Mt8 + 1]
    codes[miss] = 1
    return codes


def assert_same(got, want, what=""):
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 127, 129, 257, 385, 1003])
@pytest.mark.parametrize("L", [1, 255, 256, 257, 700])
def test_gpu_bed_sample_ibs_equals_host(tmp_path, n, L):
    from eagleeverything_amd import r_api, rcpp_api, synth
    for lost in (False, True):
        Mt8, miss = make_panel(n, L, 1000 * n + L, lost=lost)
        bed = synth.write_bed(str(tmp_path / ("p%d" % lost)), Mt8, missing=miss)
        before = open(bed, "rb").read()
        got = rcpp_api.bed_sample_ibs(bed, (n, L))
        codes = r_api.read_bed_codes(bed, (n, L))
        assert np.array_equal(codes, codes_of(Mt8, miss))
        want = r_api.bed_ibs_host(codes)
        assert_same(got, want, "lost=%s" % lost)
        assert open(bed, "rb").read() == before                                # the input is only read
        ncalled, ibs0, hethet, hetsum, dist = got
        phi = r_api.king_from_pair_counts(ibs0, hethet, hetsum)
        assert np.array_equal(np.diagonal(ncalled), (~miss).sum(axis=0))
        if L >= 2:
            assert ncalled.max() <= L - 1                                      # marker 0 counts for nobody
            if not lost:
                assert ncalled.min() >= 1                                      # marker 1 counts for every pair
        if lost:
            assert not np.any(ncalled[n - 1]) and not np.any(ncalled[:, n - 1])
            assert np.all(np.isnan(phi[n - 1])) and np.all(dist[n - 1] == NO_OVERLAP) and np.all(dist[:, n - 1] == NO_OVERLAP)
        if n >= 2 and not (lost and n == 2):
            assert dist[0, 1] == 0 or ncalled[0, 1] == 0
            assert hetsum[0, 1] == 0 or phi[0, 1] == 0.5                       # the duplicate pair, whatever is missing in either copy
            if L >= 255:
                assert phi[0, 1] == 0.5 and phi[1, 0] == 0.5 and 0 < ncalled[0, 1] < min(ncalled[0, 0], ncalled[1, 1])


def test_gpu_bed_sample_ibs_on_the_384_row_syrk(tmp_path):
    """pad256(n) >= 3072: the four products run on k_syrk_f4w's 384 x 256 tiles."""
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L = 3075, 300
    Mt8, miss = make_panel(n, L, 3075)
    bed = synth.write_bed(str(tmp_path / "wide"), Mt8, missing=miss)
    assert_same(rcpp_api.bed_sample_ibs(bed, (n, L)), r_api.bed_ibs_host(codes_of(Mt8, miss)))


@pytest.mark.parametrize("n", [5, 1003])
def test_gpu_bed_sample_ibs_ignores_pad_bits(tmp_path, n):
    """The unused bit pairs of every row's last byte set to 11 (PLINK never writes that, but nothing forbids it): the same results."""
    from eagleeverything_amd import rcpp_api, synth
    L = 300
    Mt8, miss = make_panel(n, L, 7 + n)
    bed = synth.write_bed(str(tmp_path / "clean"), Mt8, missing=miss)
    clean = rcpp_api.bed_sample_ibs(bed, (n, L))
    rb = (n + 3) // 4
    raw = np.frombuffer(open(bed, "rb").read(), dtype=np.uint8).copy()
    rows = raw[3:].reshape(L, rb)
    assert n % 4 and not np.any(rows[:, -1] >> (2 * (n % 4)))
    rows[:, -1] |= (0xFF << (2 * (n % 4))) & 0xFF
    dirty = str(tmp_path / "dirty.bed")
    open(dirty, "wb").write(raw.tobytes())
    assert open(dirty, "rb").read() != open(bed, "rb").read()
    assert_same(rcpp_api.bed_sample_ibs(dirty, (n, L)), clean)


def test_gpu_bed_sample_ibs_windows_give_the_same_integers(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L = 257, 700
    Mt8, miss = make_panel(n, L, 257700)
    bed = synth.write_bed(str(tmp_path / "w"), Mt8, missing=miss)
    want = r_api.bed_ibs_host(codes_of(Mt8, miss))
    rb = (n + 3) // 4
    for mem, at_least in ((8.0, 1), (4 * 153 * rb / 1e9, 3), (4 * 256 * rb / 1e9, 3), (4 * 1 * rb / 1e9, L)):   # the last: one marker per window
        cap = min(67108864.0, mem * 1e9 / 4.0)                                 # the library's arithmetic: a quarter of the budget per window
        w = max(1, min(L, int(cap) // rb))
        assert -(-L // w) >= at_least and (at_least == 1) == (w == L)
        assert_same(rcpp_api.bed_sample_ibs(bed, (n, L), max_memory_in_Gbytes=mem), want, "mem=%g" % mem)


def test_gpu_bed_sample_ibs_include_and_min_overlap(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L = 129, 700
    Mt8, miss = make_panel(n, L, 129700)
    bed = synth.write_bed(str(tmp_path / "all"), Mt8, missing=miss)
    rng = np.random.default_rng(5)
    inc = rng.random(L) < 0.5
    inc[:2] = True
    sub = synth.write_bed(str(tmp_path / "sub"), np.ascontiguousarray(Mt8[inc]), missing=miss[inc])
    Ls = int(inc.sum())
    want = rcpp_api.bed_sample_ibs(sub, (n, Ls))
    assert_same(rcpp_api.bed_sample_ibs(bed, (n, L), include=inc), want)
    assert_same(rcpp_api.bed_sample_ibs(bed, (n, L), include=inc.astype(np.uint8), max_memory_in_Gbytes=4 * 100 * 33 / 1e9), want)
    assert_same(want, r_api.bed_ibs_host(codes_of(Mt8, miss), include=inc))
    none = rcpp_api.bed_sample_ibs(bed, (n, L), include=np.zeros(L, dtype=bool))
    assert not any(np.any(m) for m in none[:4])
    off = ~np.eye(n, dtype=bool)
    assert np.all(none[4][off] == NO_OVERLAP) and np.all(none[4] == NO_OVERLAP)
    for min_overlap in (2, 520, L + 1):
        got = rcpp_api.bed_sample_ibs(bed, (n, L), min_overlap=min_overlap)
        assert_same(got, r_api.bed_ibs_host(codes_of(Mt8, miss), min_overlap=min_overlap), "min_overlap=%d" % min_overlap)
    assert np.all(got[4] == NO_OVERLAP)
    some = rcpp_api.bed_sample_ibs(bed, (n, L), min_overlap=520)[4]
    assert np.any(some == NO_OVERLAP) and np.any(some != NO_OVERLAP)          # 520 lies inside the range of the overlaps
    with pytest.raises(rcpp_api.EagleError):
        rcpp_api.bed_sample_ibs(bed, (n, L + 1))
    with pytest.raises(rcpp_api.EagleError):
        rcpp_api.bed_sample_ibs(bed, (n, L), min_overlap=0)


def test_gpu_bed_sample_ibs_without_missing_equals_sample_ibs(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L = 130, 300
    rng = np.random.default_rng(130)
    Mt8 = rng.integers(-1, 2, size=(L, n)).astype(np.int8)
    bed = synth.write_bed(str(tmp_path / "full"), Mt8)
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(tmp_path))
    old0, oldh = rcpp_api.sample_ibs(geno["asciifileM"], (n, L))
    ncalled, ibs0, hethet, hetsum, dist = rcpp_api.bed_sample_ibs(bed, (n, L))
    assert np.array_equal(ibs0, old0) and np.array_equal(hethet, oldh)
    assert np.all(ncalled == L)
    h = np.diagonal(hethet)
    assert np.array_equal(hetsum, h[:, None] + h[None, :])
    assert np.array_equal(dist.astype(np.int64), r_api.knn_distance(old0, oldh).astype(np.int64))    # Linc / N = 1
    assert np.array_equal(r_api.king_from_pair_counts(ibs0, hethet, hetsum), r_api.king_from_counts(old0, oldh))


@pytest.mark.parametrize("n", [1, 5, 257, 1003])
def test_gpu_knn_rows_dist_equals_host(tmp_path, n):
    from eagleeverything_amd import r_api, rcpp_api, synth
    L = 24                                                                     # few markers: ties everywhere
    Mt8, miss = make_panel(n, L, 24 + n, lost=n >= 5)
    if n >= 5:
        Mt8 = Mt8.copy()
        Mt8[:, 3] = Mt8[:, 0]                                                  # three copies of one individual
    bed = synth.write_bed(str(tmp_path / "k"), Mt8, missing=miss)
    dist = rcpp_api.bed_sample_ibs(bed, (n, L), min_overlap=3)[4]
    assert np.array_equal(dist, r_api.bed_ibs_host(codes_of(Mt8, miss), min_overlap=3)[4])
    if n >= 5:
        dist = dist.copy()
        dist[2, :] = 7                                                         # a row of one value: index order alone decides
        dist[4, 1::2] = 0                                                      # planted equal distances next to large ones
        dist[4, 0] = 0xFFFFFFFD
    for K in sorted({1, max(1, min(n - 1, 256)), min(n + 2, 256), 256}):
        got = rcpp_api.knn_rows_dist(dist, K)
        assert got.dtype == np.int32 and got.shape == (n, K)
        assert np.array_equal(got, r_api.knn_rows_host(dist, K)), K
    if n >= 5:
        keff = min(256, n - 1)
        assert got[2, :keff].tolist() == [j for j in range(n) if j != 2][:keff]
        assert got[4, :2].tolist() == [1, 3]
        if keff == n - 1:
            assert got[0, keff - 1] == n - 1                                   # no overlap: after every distance
            if n > 5:
                assert got[4, :3].tolist() == [1, 3, 5] and got[4, keff - 2:keff].tolist() == [0, n - 1]


def test_gpu_knn_rows_keeps_its_results():
    from eagleeverything_amd import r_api, rcpp_api
    n = 300
    rng = np.random.default_rng(300)
    G = rng.integers(-1, 2, size=(n, 24)).astype(np.int64)
    G[7] = G[2]
    ibs0 = ((G * G) @ (G * G).T - G @ G.T) // 2
    hethet = (1 - G * G) @ (1 - G * G).T
    ibs0, hethet = ibs0.astype(np.int32), hethet.astype(np.int32)
    got = rcpp_api.knn_rows(ibs0, hethet, 40)
    assert np.array_equal(got, r_api.knn_rows_host(r_api.knn_distance(ibs0, hethet), 40))
    assert got[2, 0] == 7 and got[7, 0] == 2


def duplicates_panel(tmp_path):
    """n = 64: 48 unrelated individuals and 8 of them written twice, 20 % of every copy's genotypes masked independently."""
    from eagleeverything_amd import synth
    n, L = 64, 400
    rng = np.random.default_rng(64)
    p = rng.uniform(0.2, 0.5, size=L)
    G = rng.binomial(2, p[None, :], size=(56, L)).astype(np.int8) - 1
    G = np.concatenate([G, G[:8]], axis=0)                                     # individual 56 + t is a copy of individual t
    mask = np.zeros((n, L), dtype=bool)
    for i in list(range(8)) + list(range(56, 64)):
        mask[i] = rng.random(L) < 0.2
    bed = synth.write_bed(str(tmp_path / "dups"), np.ascontiguousarray(G.T), missing=mask.T)
    return bed, n, L


def test_gpu_relatedness_from_the_bed_file_finds_masked_duplicates(tmp_path):
    from eagleeverything_amd import r_api
    bed, n, L = duplicates_panel(tmp_path)
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(tmp_path))
    truth = [[t, 56 + t] for t in range(8)]
    rel = r_api.Relatedness(geno, bed=bed[:-4])                                # the fileset's prefix
    assert rel["kinship"].shape == (n, n) and rel["ncalled"].shape == (n, n) and rel["ncalled"].dtype == np.int32
    assert all(rel["kinship"][i, j] == 0.5 for i, j in truth)
    dup = [pr for pr, deg in zip(rel["pairs"].tolist(), rel["degree"]) if deg == "duplicate"]
    assert dup == truth and all(v == 0.5 for v, deg in zip(rel["phi"].tolist(), rel["degree"]) if deg == "duplicate")
    assert all(rel["ncalled"][i, j] < L for i, j in truth)
    old = r_api.Relatedness(geno)
    assert "ncalled" not in old
    with np.errstate(invalid="ignore"):
        assert not np.any(np.triu(old["kinship"] >= 0.45, k=1))               # the het-filled panel: no duplicate found
    assert all(old["kinship"][i, j] < 0.45 for i, j in truth)
    # a filtered panel: include names its markers in the .bed file
    keep = np.arange(0, L, 2)
    sub = {"asciifileM": geno["asciifileM"], "asciifileMt": geno["asciifileMt"], "dim_of_ascii_M": [n, keep.size]}
    half = r_api.Relatedness(sub, bed=bed, include=keep)
    codes = r_api.read_bed_codes(bed, (n, L))
    want = r_api.bed_ibs_host(codes, include=keep)
    assert np.array_equal(half["ncalled"], want[0]) and np.array_equal(half["ibs0"], want[1])
    assert all(half["kinship"][i, j] == 0.5 for i, j in truth)
    with pytest.raises(ValueError):
        r_api.Relatedness(sub, bed=bed)


def test_gpu_impute_bed_pairwise_and_default(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L, k, K = 150, 100, 5, 32
    rng = np.random.default_rng(21)
    founders = rng.integers(-1, 2, size=(6, L))
    M = np.repeat(founders, 25, axis=0)
    M = np.where(rng.random(M.shape) < 0.05, rng.integers(-1, 2, size=M.shape), M).astype(np.int8)
    miss = rng.random((L, n)) < 0.2
    bed = synth.write_bed(str(tmp_path / "panel"), np.ascontiguousarray(M.T), missing=miss)
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(tmp_path))
    codes = r_api.read_bed_codes(bed, (n, L))

    res = r_api.ImputeBed(bed, geno, str(tmp_path / "pw" / "p"), k=k, K=K, pairwise=True, min_overlap=10)
    nbr = r_api.knn_rows_host(r_api.bed_ibs_host(codes, min_overlap=10)[4], K)
    rows, counts = r_api.impute_knn_host(codes, nbr, k, 1)
    assert open(res["bed"], "rb").read() == HEAD + rows.tobytes() and np.array_equal(res["counts"], counts)
    assert res["n_missing"] == int(miss.sum())

    res0 = r_api.ImputeBed(bed, geno, str(tmp_path / "def" / "p"), k=k, K=K)
    ibs0, hethet = rcpp_api.sample_ibs(geno["asciifileM"], (n, L))
    nbr0 = r_api.knn_rows_host(r_api.knn_distance(ibs0, hethet), K)
    rows0, counts0 = r_api.impute_knn_host(codes, nbr0, k, 1)
    assert open(res0["bed"], "rb").read() == HEAD + rows0.tobytes() and np.array_equal(res0["counts"], counts0)
    assert not np.array_equal(nbr, nbr0)                                       # the two distances do rank differently here
    for ext in (".bim", ".fam"):
        assert open(res["bed"][:-4] + ext, "rb").read() == open(bed[:-4] + ext, "rb").read()
