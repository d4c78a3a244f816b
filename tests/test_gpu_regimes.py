"""The n-sized kernels on the GPU at every row-length regime and at their capacities.

The other test_gpu_*.py stop at n = 1,003 individuals (one case each at 2,049 and 3,075), so a .bed row was never longer than 251 bytes
(769 in those two) and no LDS request that grows with n came near its maximum.  Here n alone is large -- L stays between 1 and 300 markers
-- and every case first asserts the regime it is meant to run from arithmetic restated in tests/regimes_truth.py (tests/test_regimes_host.py
and the test_*_abi.py pin that arithmetic to the source text), then prints it:

  A. rows of rb = ceil(n / 4) bytes: k_bed_impute's two thread layouts (rb < 256 / rb >= 256) and the three terms of its rows per block,
     up to the full 60 KiB stage at n = 245,760; k_bed_impute_ldknn's second trip of its 512-thread column loops; every other eagle_bed_*
     entry point at rb = 256, 1,025 and 16,385.
  B. dynamic LDS sized by n at the accepted maximum: 4 n bytes of k_knn_rows / k_knn_rows_dist up to 128 KiB, 12.5 n bytes of
     k_bed_impute_ldknn at 150 KiB; the epistasis scan at EAGLE_EPI_MAX_N.
  C. the second batch of the 65,535-unit loops: offspring chunks of the parentage search and word batches of eagle_dev_plane_gather.

Truth is r_api's host restatements (tests/test_*_host.py pin them to plain loops); where one is too heavy at the shape it is restated per
missing genotype (regimes_truth.impute_knn_sparse) or per sampled row (regimes_truth.knn_row).  Integers and bytes: every comparison is ==."""
import functools
import time

import numpy as np
import pytest

import regimes_truth as R
from test_gpu_bed import decode_bed, text_bytes
from test_gpu_epistasis import check_pairs, same_bits, threshold
from test_gpu_mendel import same_rows, trio_list
from test_gpu_roh import same as same_tables

pytestmark = pytest.mark.gpu

KNN_CAPACITY_N = 32768                    # EAGLE_KNN_MAX_N: 128 KiB of dynamic LDS, a 4 GiB matrix


def say(**regime):
    print("regime: " + ", ".join("%s=%s" % kv for kv in regime.items()))


# ================================================================================================ A. k_bed_impute
@functools.lru_cache(maxsize=4)
def impute_panel(n, L, small):
    """2 % missing; with three markers or more: marker 0 with 40 % missing (neighbours that are themselves missing), marker 1 without a
    missing call (a row copy) and, at the small shapes, marker 2 with every call missing (the fallback to het)."""
    many = L >= 3
    codes = R.codes_panel(n, L, seed=7 * n + L, rate=0.02, dense=0 if many else None, full=1 if many else None,
                          empty=2 if many and small else None)
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=4)
def impute_table(n, K):
    nbr = R.neighbour_table(n, K, seed=n + K)
    nbr.setflags(write=False)
    return nbr


def impute_case(tmp_path, n, L, K, k, small):
    from eagleeverything_amd import r_api, rcpp_api
    rb = R.row_bytes(n)
    rows_per_block = R.imp_rows_per_block(rb)
    blocks = -(-L // rows_per_block)
    codes, nbr = impute_panel(n, L, small), impute_table(n, K)
    bed = R.write_codes(str(tmp_path / "in.bed"), codes)
    before = open(bed, "rb").read()
    out = str(tmp_path / "out.bed")
    counts = rcpp_api.bed_impute_knn(bed, (n, L), nbr, k, 1, out)
    want_rows, want_counts = R.impute_knn_sparse(codes, nbr, k, 1)
    if n * L * K <= 20000000:                                                  # r_api's own restatement where it takes a fraction of a second
        host_rows, host_counts = r_api.impute_knn_host(codes, nbr, k, 1)
        assert np.array_equal(host_rows, want_rows) and np.array_equal(host_counts, want_counts)
    got = open(out, "rb").read()
    assert len(got) == 3 + L * rb and got[:3] == R.HEAD
    raw = np.frombuffer(got, dtype=np.uint8)[3:].reshape(L, rb)
    assert np.array_equal(raw, want_rows), np.argwhere(raw != want_rows)[:5].tolist()
    assert counts.dtype == np.int32 and counts.shape == (L, 2) and np.array_equal(counts, want_counts)
    assert np.array_equal(counts.sum(axis=1), (codes == 1).sum(axis=1))        # the pad's missing code is not counted
    if n % 4:
        assert not (raw[:, -1] >> (2 * (n % 4))).any()                         # the pad bit pairs go out as 00
    assert not (r_api.read_bed_codes(out, (n, L)) == 1).any()
    assert open(bed, "rb").read() == before                                    # the input is only read
    if L >= 3:
        src = np.frombuffer(before, dtype=np.uint8)[3:].reshape(L, rb)
        keep = 0xff >> (2 * (-n % 4))
        assert counts[1].tolist() == [0, 0] and np.array_equal(raw[1, :-1], src[1, :-1]) and raw[1, -1] == src[1, -1] & keep
        hit = (codes[0] == 1) & (nbr[:, 0] >= 0)
        assert (codes[0][nbr[hit, 0]] == 1).any()                              # a first neighbour that is itself missing at the marker
        if small:
            assert counts[2].tolist() == [0, n] and (r_api.read_bed_codes(out, (n, L))[2] == 2).all()
    assert counts[:, 0].sum() > 0 and (nbr == -1).any()
    return rb, rows_per_block, blocks


IMPUTE_SMALL = {1020: (255, False, 64), 1021: (256, True, 64), 1024: (256, True, 64), 1025: (257, True, 63), 4099: (1025, True, 15)}
IMPUTE_SMALL_CASES = [(n, L, K, k) for n in IMPUTE_SMALL for L in (1, 3, 300) for K in (8, 256) for k in (1, 5)]
IMPUTE_SMALL_CASES += [(4099, 301, 8, 5), (4099, 301, 256, 1)]                 # 300 = 20 x 15 rows: one more marker leaves a short last block


@pytest.mark.parametrize("n,L,K,k", IMPUTE_SMALL_CASES)
def test_gpu_bed_impute_on_both_sides_of_the_256_byte_row(tmp_path, n, L, K, k):
    """rb < 256: a thread is a (row, byte column) pair; rb >= 256: every thread walks the columns tid, tid + 256, ... of every row."""
    rb, walk, rows_per_block = IMPUTE_SMALL[n]
    assert rb == R.row_bytes(n) and walk == (rb >= R.IMP_WALK_RB) and rows_per_block == 16384 // rb and R.imp_rows_regime(rb) == "16384/rb"
    got = impute_case(tmp_path, n, L, K, k, small=True)
    assert got[:2] == (rb, rows_per_block)
    if L >= 300:
        assert got[2] > 1 and (L % rows_per_block != 0 or (n, L) == (4099, 300))      # several blocks, the last one short
    say(n=n, rb=rb, layout="columns tid + 256 t" if walk else "(row, column) pairs", second_trip=rb > 256, rows_per_block=rows_per_block,
        blocks=got[2], last_block_rows=L - (got[2] - 1) * rows_per_block, K=K, k=k)


@pytest.mark.parametrize("n,rb,quotient", [(32768, 8192, 2), (32769, 8193, 1), (65533, 16384, 1), (65536, 16384, 1), (65540, 16385, 0)])
def test_gpu_bed_impute_where_16384_over_rb_reaches_one_and_zero(tmp_path, n, rb, quotient):
    """A block holds two rows at rb = 8,192 and one from 8,193 on; at rb = 16,385 the term 16384 / rb is 0 and only its max(1, .) keeps the
    block alive."""
    L, K = 5, 8
    assert rb == R.row_bytes(n) and quotient == 16384 // rb and R.imp_rows_regime(rb) == ("16384/rb" if quotient else "1")
    rows_per_block = max(1, quotient)
    got = impute_case(tmp_path, n, L, K, 5, small=False)
    assert got == (rb, rows_per_block, -(-L // rows_per_block))
    say(n=n, rb=rb, quotient_16384_over_rb=quotient, rows_per_block=rows_per_block, blocks=got[2], columns_per_thread=R.trips(rb, 256),
        last_byte_holds=(n - 1) % 4 + 1)


@pytest.mark.parametrize("n,last", [(245757, 1), (245760, 4)])
def test_gpu_bed_impute_with_the_stage_full(tmp_path, n, last):
    """EAGLE_IMPUTE_MAX_N: the row is the whole 60 KiB stage, the last byte holds one individual or four."""
    L, K = 3, 8
    rb = R.row_bytes(n)
    assert rb == R.IMP_STAGE_BYTES == 61440 and n - 4 * (rb - 1) == last and n <= 4 * R.IMP_STAGE_BYTES
    got = impute_case(tmp_path, n, L, K, 5, small=False)
    assert got == (rb, 1, L)
    say(n=n, rb=rb, stage_bytes=R.IMP_STAGE_BYTES, rows_per_block=1, blocks=L, columns_per_thread=R.trips(rb, 256), last_byte_holds=last)


# ================================================================================================ A / B. k_bed_impute_ldknn
@pytest.mark.parametrize("n,full", [(2045, False), (2049, True), (8193, False), (12285, False), (12287, False), (12288, True)])
def test_gpu_bed_impute_ldknn_second_trip_and_150_kib(tmp_path, n, full):
    """512 threads over rb byte columns: a second trip from n = 2,049 on; 12.5 n bytes of LDS, 150 KiB (one block a CU) at the accepted
    maximum n = 12,288.  Partners: the 16 markers on either side."""
    from eagleeverything_amd import r_api, rcpp_api
    L = 40
    l, k, min_overlap = (32, 64, 4) if full else (7, 5, 2)
    rb, lds = R.row_bytes(n), R.ldk_lds_bytes(n)
    column_trips = R.trips(rb, R.LDK_THREADS)
    assert column_trips == {2045: 1, 2049: 2, 8193: 5, 12285: 6, 12287: 6, 12288: 6}[n] and (column_trips >= 2) == (n > 2048)
    assert lds == {2045: 25600, 2049: 25656, 8193: 102456, 12285: 153600, 12287: 153600, 12288: 153600}[n] and lds <= 150 * 1024
    assert n <= rcpp_api.LDKNN_MAX_N == 12288
    codes, full_codes = R.cluster_panel(n, L, seed=n, rate=0.002)              # copies of 8 founders: which neighbours vote decides the code
    codes[1] = full_codes[1]                                                   # a marker without a missing call
    codes[2::4, n - 1] = codes[6, 0] = 1                                       # the last individual: byte column rb - 1, the last trip's
    part = np.ascontiguousarray(R.ld_neighbours(L)[:, :l])
    bed = R.write_codes(str(tmp_path / "in.bed"), codes)
    before = open(bed, "rb").read()
    out = str(tmp_path / "out.bed")
    counts = rcpp_api.bed_impute_ldknn(bed, (n, L), part, k, 1, min_overlap, out)
    want_rows, want_counts = r_api.impute_ldknn_host(codes, part, k, 1, min_overlap)
    raw = np.frombuffer(open(out, "rb").read(), dtype=np.uint8)
    assert raw.size == 3 + L * rb and bytes(raw[:3]) == R.HEAD
    raw = raw[3:].reshape(L, rb)
    assert np.array_equal(raw, want_rows), np.argwhere(raw != want_rows)[:5].tolist()
    assert counts.dtype == np.int32 and np.array_equal(counts, want_counts) and np.array_equal(counts.sum(axis=1), (codes == 1).sum(axis=1))
    assert counts[1].tolist() == [0, 0] and counts[:, 0].sum() > 10 * counts[:, 1].sum() and open(bed, "rb").read() == before
    if n % 4:
        assert not (raw[:, -1] >> (2 * (n % 4))).any()
    assert ((n - 1) // 4) // R.LDK_THREADS == column_trips - 1                 # ten genotypes filled in the last trip's columns ...
    last = (want_rows[2::4, rb - 1] >> (2 * ((n - 1) % 4))) & 3
    assert (last == full_codes[2::4, n - 1]).mean() >= 0.8 and len(set(last.tolist())) >= 2   # ... from their own founder's copies, not all het
    say(n=n, rb=rb, column_trips=column_trips, lds_bytes=lds, l=l, k=k, min_overlap=min_overlap)


# ================================================================================================ A. every other eagle_bed_* entry point
ROW_NS = {1021: 256, 4099: 1025, 65540: 16385}
ROW_CASES = [(n, L) for n in ROW_NS for L in (1, 5)]
SQUARE_CASES = [(n, L) for n in (1021, 4099) for L in (1, 5)]


@functools.lru_cache(maxsize=2)
def row_panel(n, L):
    codes = R.codes_panel(n, L, seed=3 * n + L, rate=0.05)
    codes.setflags(write=False)
    return codes


def row_case(tmp_path, n, L):
    rb = ROW_NS[n]
    assert rb == R.row_bytes(n) and rb >= 256
    say(n=n, L=L, rb=rb)
    codes = row_panel(n, L)
    return codes, R.write_codes(str(tmp_path / "p.bed"), codes)


@pytest.mark.parametrize("n,L", ROW_CASES)
def test_gpu_bed_counts_at_long_rows(tmp_path, n, L):
    """bed_marker_counts, bed_sample_counts and bed_group_counts (K = 3 and the largest, 64)."""
    from eagleeverything_amd import r_api, rcpp_api
    codes, bed = row_case(tmp_path, n, L)
    by = lambda axis: np.stack([(codes == c).sum(axis=axis) for c in (0, 2, 3, 1)], axis=1).astype(np.int32)      # noqa: E731
    got = rcpp_api.bed_marker_counts(bed, (n, L))
    assert got.dtype == np.int32 and np.array_equal(got, by(1)) and (got.sum(axis=1) == n).all()
    got = rcpp_api.bed_sample_counts(bed, (n, L))
    assert got.dtype == np.int32 and np.array_equal(got, by(0)) and (got.sum(axis=1) == L).all()
    rng = np.random.default_rng(n + L)
    for K in (3, 64):
        labels = rng.integers(-1, K, size=n)
        labels[[0, n - 1]] = K - 1, 0
        got = rcpp_api.bed_group_counts(bed, (n, L), labels, K)
        assert got.dtype == np.int32 and got.shape == (L, K, 4) and np.array_equal(got, r_api.bed_group_counts_host(codes, labels, K)), K
        assert np.array_equal(got.sum(axis=(1, 2)), np.full(L, (labels >= 0).sum()))


@pytest.mark.parametrize("n,L", ROW_CASES)
def test_gpu_bed_roh_and_ld_window_at_long_rows(tmp_path, n, L):
    from eagleeverything_amd import r_api, rcpp_api
    codes, bed = row_case(tmp_path, n, L)
    prm = dict(w=min(L, 2), win_het=0, win_miss=1, min_snp=min(L, 2))
    want = r_api.roh_host(r_api.roh_classes_bed(codes), **prm)
    same_tables(rcpp_api.bed_roh(bed, (n, L), **prm), want, (n, L))
    assert want[1].shape[0] > n // 8 and want[1][:, 0].max() >= n - 8         # segments up to the last individuals
    window, t = 4, 0.5 / n                                                     # r2 of unlinked markers is about 1 / n
    mask, npairs = rcpp_api.bed_ld_window(bed, (n, L), window, t, None, 1, return_pairs=True)
    want_mask = r_api.bed_ld_mask_host(codes, window, t, None, 1)
    assert mask.dtype == np.uint64 and mask.shape == want_mask.shape == (L, 1) and np.array_equal(mask, want_mask)
    assert npairs == int(np.unpackbits(np.ascontiguousarray(want_mask).view(np.uint8)).sum()) and (L == 1 or npairs > 0)


@pytest.mark.parametrize("n,L", ROW_CASES)
def test_gpu_bed_mendel_at_long_rows(tmp_path, n, L):
    from eagleeverything_amd import r_api, rcpp_api
    codes, bed = row_case(tmp_path, n, L)
    g, called = r_api.ibd_genotypes_bed(codes)
    trios = np.concatenate((trio_list(n, 130, seed=n + L), np.array([(n - 1, n - 2, n - 3), (n - 4, -1, n - 1), (0, n - 1, n - 5)],
                                                                     dtype=np.int32)))
    want_tab, want_marker = r_api.mendel_host(g, called, trios)
    tab, marker = rcpp_api.bed_mendel(bed, (n, L), trios)
    same_rows(tab, want_tab, (n, L, "trio"))
    same_rows(marker, want_marker, (n, L, "marker"))
    assert tab[:, 5].sum() > 0 and tab[:, 5].sum() == marker.sum()
    rcpp_api.drop_cache()


@pytest.mark.parametrize("n,L", ROW_CASES)
def test_gpu_bed_decode_at_long_rows(tmp_path, n, L):
    """create_ascii_from_bed: k_bed_decode's M.ascii and Mt.ascii."""
    from eagleeverything_amd import rcpp_api
    codes, bed = row_case(tmp_path, n, L)
    digits, missing = decode_bed(bed, n, L)
    assert np.array_equal(missing, codes == 1)
    fM, fMt = str(tmp_path / "M.ascii"), str(tmp_path / "Mt.ascii")
    assert rcpp_api.create_ascii_from_bed(bed, fM, fMt, 8.0, [n, L]) == int(missing.sum()) > 0
    assert open(fMt, "rb").read() == text_bytes(digits)
    assert open(fM, "rb").read() == text_bytes(np.ascontiguousarray(digits.T))
    rcpp_api.drop_cache()


@pytest.mark.parametrize("n,L", SQUARE_CASES)
def test_gpu_bed_sample_ibs_at_long_rows(tmp_path, n, L):
    from eagleeverything_amd import r_api, rcpp_api
    codes, bed = row_case(tmp_path, n, L)
    got = rcpp_api.bed_sample_ibs(bed, (n, L))
    want = r_api.bed_ibs_host(codes)
    for name, a, b in zip(("ncalled", "ibs0", "hethet", "hetsum", "dist"), got, want):
        assert a.dtype == b.dtype and a.shape == (n, n) and np.array_equal(a, b), (name, np.argwhere(a != b)[:5].tolist())
    assert (L > 1 or (got[4] == rcpp_api.DIST_NO_OVERLAP).any()) and got[0][n - 1, n - 1] == (codes[:, n - 1] != 1).sum()


@pytest.mark.parametrize("n,L", SQUARE_CASES)
def test_gpu_bed_ibd_all_pairs_at_long_rows(tmp_path, n, L):
    from eagleeverything_amd import r_api, rcpp_api
    codes, bed = row_case(tmp_path, n, L)
    g, called = r_api.ibd_genotypes_bed(codes)
    prm = dict(mode=2, min_snp=min(L, 3), merge_min=1)
    P = n * (n - 1) // 2
    want_tab, want_seg = r_api.ibd_host(g, called, **prm)
    tab, seg = rcpp_api.bed_ibd(bed, (n, L), seg_cap=P, **prm)
    assert tab.dtype == np.int64 and tab.shape == (P, 4) and np.array_equal(tab, want_tab)
    assert seg.dtype == np.int32 and seg.shape == want_seg.shape and np.array_equal(seg, want_seg)
    assert 0 < seg.shape[0] <= P and seg[:, 1].max() == n - 1
    rcpp_api.drop_cache()


@pytest.mark.parametrize("n,L", SQUARE_CASES)
def test_gpu_bed_parentage_at_long_rows(tmp_path, n, L):
    from eagleeverything_amd import r_api, rcpp_api
    codes, bed = row_case(tmp_path, n, L)
    g, called = r_api.ibd_genotypes_bed(codes)
    sires, dams, off = np.array([0, 1, 2, n - 1, n - 2]), np.array([3, 4, 5, n - 3, n - 4]), np.arange(6, n - 4)
    want = r_api.parentage_host(g, called, off, sires, dams, 1)
    got = rcpp_api.bed_parentage(bed, (n, L), off, sires, dams, None, 1)
    same_rows(got, want, (n, L))
    assert (got[:, 0, 3] >= 1).sum() > off.size // 2 and (L == 1 or len(set(got[:, 0, 0].tolist())) > 2)
    rcpp_api.drop_cache()


# ================================================================================================ B. 4 n bytes of LDS
_DIST = {}


def dist_of(n):
    """One matrix at a time: 1 GiB at n = 16,385, 4 GiB at 32,768."""
    if n not in _DIST:
        _DIST.clear()
        _DIST[n] = R.dist_matrix(n)
    return _DIST[n]


@pytest.mark.parametrize("K", [1, 256])                                        # the upper decorator varies fastest: both K on one matrix
@pytest.mark.parametrize("n", [16385, KNN_CAPACITY_N])
def test_gpu_knn_rows_dist_past_64_kib_and_at_the_capacity(n, K):
    """16,385 is the first n whose row passes 64 KiB of dynamic LDS; EAGLE_KNN_MAX_N = 32,768 asks for 128 KiB."""
    from eagleeverything_amd import rcpp_api
    t0 = time.time()
    lds = R.knn_lds_bytes(n)
    assert lds == 4 * n and (lds > 64 * 1024) and n <= 32768 and (n != 32768 or lds == 128 * 1024)
    dist = dist_of(n)
    t1 = time.time()
    got = rcpp_api.knn_rows_dist(dist, K)
    t2 = time.time()
    assert got.dtype == np.int32 and got.shape == (n, K) and got.min() >= 0 and got.max() < n
    assert not (got == np.arange(n)[:, None]).any()
    rows = R.sampled_rows(n)
    for i in rows.tolist():
        assert np.array_equal(got[i], R.knn_row(dist[i], i, K)), (n, K, i)
    assert np.array_equal(dist[rows], R.dist_rows(rows, n))                    # the matrix is what the builder says: only read
    say(n=n, K=K, lds_bytes=lds, entries_per_thread=R.trips(n, R.KNN_THREADS), sampled_rows=rows.size, build_s=round(t1 - t0, 2),
        call_s=round(t2 - t1, 2), check_s=round(time.time() - t2, 2))
    if K == 256:
        _DIST.clear()


def test_gpu_knn_rows_past_64_kib():
    """k_knn_rows (ibs0, hethet) at n = 16,385: d = 4 ibs0 + h_i + h_j - 2 hethet formed in the kernel, 65,540 bytes of LDS."""
    from eagleeverything_amd import rcpp_api
    n = 16385
    lds = R.knn_lds_bytes(n)
    assert lds == 65540 > 64 * 1024
    ibs0, hethet = R.ibs_matrices(n)
    h = np.diagonal(hethet).astype(np.int64)
    rows = R.sampled_rows(n, seed=1)
    for K in (1, 256):
        got = rcpp_api.knn_rows(ibs0, hethet, K)
        assert got.dtype == np.int32 and got.shape == (n, K) and got.min() >= 0 and not (got == np.arange(n)[:, None]).any()
        for i in rows.tolist():
            d = (4 * ibs0[i].astype(np.int64) + h[i] + h - 2 * hethet[i]).astype(np.int32)
            assert np.array_equal(got[i], R.knn_row(d, i, K)), (K, i)
    say(n=n, lds_bytes=lds, entries_per_thread=R.trips(n, R.KNN_THREADS), sampled_rows=rows.size)


# ================================================================================================ B. epistasis at EAGLE_EPI_MAX_N
def test_gpu_epistasis_at_the_largest_n(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L = 65535, 129
    assert n == rcpp_api.EPI_MAX_N
    rng = np.random.default_rng(5)
    M8 = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(n, L), p=[0.3, 0.4, 0.3])
    M8[:, 40], M8[:, 41], M8[:, 90] = M8[:, 3], -M8[:, 3], 1                  # a duplicate, its mirror, a monomorphic marker: undefined pairs
    y = rng.integers(-1000000, 1000001, n).astype(np.int32)
    y[0], y[n - 1] = 1000000, -1000000
    loci = rng.integers(0, L, 64)
    loci[0], loci[1], loci[5], loci[63] = 0, L - 1, loci[4], L - 1
    host = r_api.epistasis_host(M8, y, loci=loci)
    pairs = r_api.epistasis_host(M8, y, min_stat=-np.inf)
    rcpp_api.drop_cache()
    Mt = synth.write_ascii(str(tmp_path / "Mt.ascii"), np.ascontiguousarray(M8.T))
    stat, mom = rcpp_api.epistasis_loci(Mt, (n, L), y, loci)
    assert stat.shape == (L, 64) and np.array_equal(mom, host["mom"]) and same_bits(stat, host["stat"])
    assert np.isnan(stat[0, 0]) and np.isnan(stat[L - 1, 1])                   # i = j
    t = threshold(pairs)
    check_pairs(rcpp_api.epistasis_pairs(Mt, (n, L), y, min_stat=t), pairs, t)
    assert 0 < pairs["ntested"] < L * (L - 1) // 2
    say(n=n, L=L, loci=64, ntested=pairs["ntested"], hits_at=t)
    rcpp_api.drop_cache()


# ================================================================================================ C. the second batch of 65,535
@functools.lru_cache(maxsize=1)
def second_chunk_pedigree():
    """2 sires, 2 dams and 65,536 + 5 offspring, 64 markers, nothing missing; offspring o is a child of pair o % 4 of (sire, dam) = (0, 2),
    (0, 3), (1, 2), (1, 3) (the last one of pair 1), so 65,534, 65,535, 65,536 and the last offspring have four different pairs."""
    from eagleeverything_amd import r_api
    n_o, L = 65536 + 5, 64
    rng = np.random.default_rng(9)
    par = rng.integers(-1, 2, size=(L, 4)).astype(np.int8)
    combos = np.array([(0, 2), (0, 3), (1, 2), (1, 3)])
    which = np.arange(n_o) % 4
    which[-1] = 1
    g = np.concatenate((par, R.children(par, combos[which], seed=2)), axis=1)
    off = np.arange(4, 4 + n_o, dtype=np.int32)
    want = r_api.parentage_host(g, None, off, [0, 1], [2, 3])
    for a in (g, off, want, which):
        a.setflags(write=False)
    return g, off, want, combos[which]


def second_chunk_regime(n_o):
    chunk = R.parentage_chunk(n_o, 2, 2)
    chunks = -(-n_o // chunk)
    assert chunk == R.GRID_Y == 65535 and chunks == 2 and n_o - chunk == 6
    say(n_o=n_o, chunk=chunk, chunks=chunks, second_chunk_offspring=n_o - chunk)


def check_second_chunk(got, want, true_pairs):
    same_rows(got, want, "all offspring")
    assert np.array_equal(got[:, 0, :2], true_pairs) and not got[:, 0, 2].any() and (got[:, 0, 3] == 64).all()
    edge = got[[65533, 65534, 65535, 65536, -1], 0, :2].tolist()
    assert edge[1:] == [[1, 2], [1, 3], [0, 2], [0, 3]] and edge[0] == [0, 3]         # both sides of the chunk edge, and the last row


def test_gpu_parentage_second_chunk_of_offspring(tmp_path):
    """eagle_parentage: the offspring go through k_parentage 65,535 at a time (gridDim.y); the second chunk reads and writes at o0."""
    from eagleeverything_amd import rcpp_api, synth
    g, off, want, true_pairs = second_chunk_pedigree()
    second_chunk_regime(off.size)
    L, n = g.shape
    rcpp_api.drop_cache()
    M = synth.write_ascii(str(tmp_path / "M.ascii"), np.ascontiguousarray(g.T))
    check_second_chunk(rcpp_api.parentage(M, (n, L), off, [0, 1], [2, 3]), want, true_pairs)
    rcpp_api.drop_cache()


def test_gpu_bed_parentage_second_chunk_of_offspring(tmp_path):
    from eagleeverything_amd import rcpp_api
    g, off, want, true_pairs = second_chunk_pedigree()
    second_chunk_regime(off.size)
    L, n = g.shape
    bed = R.write_codes(str(tmp_path / "p.bed"), np.array([0, 2, 3], dtype=np.uint8)[g + 1])
    check_second_chunk(rcpp_api.bed_parentage(bed, (n, L), off, [0, 1], [2, 3], None, 1), want, true_pairs)
    rcpp_api.drop_cache()


@pytest.mark.parametrize("n", [4, 68])
def test_gpu_plane_gather_second_batch_of_words(tmp_path, n):
    """eagle_dev_plane_gather takes 65,535 words of 64 markers per launch (gridDim.y).  The parentage search gathers the planes of its three
    lists over all the panel's words in one call (parentage_run in csrc/eagle_ingest.cpp; eagle_mendel's trio pass reads the planes where
    they lie and never gathers), so 64 x 65,535 + 65 markers make a second launch of two words.  Four individuals: sires 0 and 1, dam 2,
    and 3, an error-free child of (0, 2) but for the errors planted in words 65,534, 65,535, 65,536 -- the last word.  n = 68 puts 64
    individuals behind them that no list names (all hom A1), so that the planes' stride, pad64(n) = 128, is not the sub-planes', 64: the
    two base pointers of the second launch then advance by different amounts."""
    from eagleeverything_amd import r_api, rcpp_api
    L = 64 * 65535 + 65
    nwords = (L + 63) // 64
    batches = -(-nwords // R.GRID_Y)
    assert nwords == 65537 and batches == 2 and nwords - R.GRID_Y == 2 and L - 1 == 64 * 65536
    src_stride, dst_stride = (n + 63) // 64 * 64, 64
    assert (src_stride != dst_stride) == (n == 68)
    say(n=n, L=L, nwords=nwords, gather_launches=batches, words_in_second_launch=nwords - R.GRID_Y, src_stride=src_stride, dst_stride=dst_stride)
    rng = np.random.default_rng(13)
    g = rng.integers(-1, 2, size=(L, 3)).astype(np.int8)
    g = np.concatenate((g, R.children(g, [(0, 2)], seed=3)), axis=1)
    called = rng.random((L, 4)) >= 0.01
    planted = np.unique([64 * 65534 + 3, 64 * 65535 - 1, 64 * 65535, 64 * 65535 + 63, 64 * 65536, L - 1])     # the last word holds one marker
    g[planted] = (-1, 1, -1, 1)                                                # both true parents hom A1, the child hom A2
    called[planted] = True
    g[~called] = 0
    codes = np.array([0, 2, 3], dtype=np.uint8)[g + 1]
    codes[~called] = 1
    rows = np.zeros((L, R.row_bytes(n)), dtype=np.uint8)
    rows[:, 0] = r_api.pack_bed_codes(codes)[:, 0]                             # the four of them in the first byte; the others 00
    bed = str(tmp_path / "p.bed")
    with open(bed, "wb") as f:
        f.write(R.HEAD)
        f.write(rows.tobytes())
    want = r_api.parentage_host(g, called, [3], [0, 1], [2], 1)                # on the four columns the lists name
    got = rcpp_api.bed_parentage(bed, (n, L), [3], [0, 1], [2], None, 1)
    same_rows(got, want, "the one offspring")
    assert got[0, 0, :3].tolist() == [0, 2, planted.size] and got[0, 1, 0] == 1 and got[0, 1, 2] > planted.size
    assert got[0, 0, 3] == int((called[:, 0] & called[:, 2] & called[:, 3]).sum()) < L
    trios = np.array([(3, 0, 2), (3, 1, 2)], dtype=np.int32)
    want_tab, want_marker = r_api.mendel_host(g, called, trios)
    tab, marker = rcpp_api.bed_mendel(bed, (n, L), trios)
    same_rows(tab, want_tab, "trio")
    same_rows(marker, want_marker, "marker")
    assert tab[0, 5] == planted.size and (marker[planted] >= 1).all() and marker.sum() == tab[:, 5].sum()
    rcpp_api.drop_cache()
