"""CPU: the builders of tests/regimes_truth.py against r_api's restatements and plain loops, and its restated launch arithmetic against the
source text of the kernels, so that tests/test_gpu_regimes.py asserts the regimes the library really has.  No device work."""
import os
import re

import numpy as np
import pytest

import regimes_truth as R
from conftest import ROOT


def source(name):
    return open(os.path.join(ROOT, "eagleeverything_amd", "csrc", name)).read()


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_constants_are_the_source_text():
    h, imp, ldk = header(), source("eagle_impute.hip"), source("eagle_ldknn.hip")
    assert int(re.search(r"#define\s+EAGLE_IMPUTE_MAX_N\s+(\d+)L", h).group(1)) == 4 * R.IMP_STAGE_BYTES == 245760
    assert re.search(r"#define IMP_STAGE_BYTES \(EAGLE_IMPUTE_MAX_N / 4\)", imp)
    assert int(re.search(r"#define IMP_MAX_ROWS (\d+)", imp).group(1)) == R.IMP_MAX_ROWS
    assert "rb >= %d" % R.IMP_WALK_RB in imp and "dim3(%d)" % R.KNN_THREADS in imp
    assert int(re.search(r"#define LDK_THREADS (\d+)", ldk).group(1)) == R.LDK_THREADS
    assert "w0 += %d" % R.GRID_Y in source("eagle_mendel.hip") and "std::min(n_o, %dL)" % R.GRID_Y in source("eagle_ingest.cpp")


def test_rows_per_block_by_hand():
    # rb <= 64: 256 rows; then 16384 // rb; past 16384 the quotient is 0 and the block holds one row
    for rb, rows, regime in ((1, 256, "256"), (64, 256, "256"), (65, 252, "16384/rb"), (255, 64, "16384/rb"), (256, 64, "16384/rb"),
                             (257, 63, "16384/rb"), (1025, 15, "16384/rb"), (8192, 2, "16384/rb"), (8193, 1, "16384/rb"),
                             (16384, 1, "16384/rb"), (16385, 1, "1"), (61440, 1, "1")):
        assert R.imp_rows_per_block(rb) == rows and R.imp_rows_regime(rb) == regime, rb
        assert rows * rb <= R.IMP_STAGE_BYTES                                  # whole rows inside the stage
    assert R.row_bytes(245760) == R.IMP_STAGE_BYTES == 61440 and R.row_bytes(245757) == 61440
    assert R.ldk_lds_bytes(12288) == 150 * 1024 and R.ldk_lds_bytes(1003) == 12 * 1004 + 8 * 63
    assert R.knn_lds_bytes(32768) == 128 * 1024 and R.knn_lds_bytes(16384) == 64 * 1024 < R.knn_lds_bytes(16385)
    assert R.trips(512, 512) == 1 and R.trips(513, 512) == 2 and R.trips(3072, 512) == 6
    assert R.parentage_parts(2, 2) == 1 and R.parentage_parts(17, 65) == 4 and R.parentage_parts(0, 5) == 1
    assert R.parentage_chunk(65541, 2, 2) == 65535 and R.parentage_chunk(10, 2, 2) == 10


@pytest.mark.parametrize("n", [1, 4, 5, 1021])
def test_write_codes_round_trip(tmp_path, n):
    from eagleeverything_amd import r_api, synth
    L = 7
    codes = R.codes_panel(n, L, seed=n, rate=0.1, dense=0, full=1, empty=2)
    assert (codes[1] != 1).all() and (codes[2] == 1).all() and (n < 100 or (codes[0] == 1).mean() > 0.3)
    bed = R.write_codes(str(tmp_path / "a.bed"), codes)
    assert np.array_equal(r_api.read_bed_codes(bed, (n, L)), codes)
    raw = np.frombuffer(open(bed, "rb").read(), dtype=np.uint8)
    assert bytes(raw[:3]) == R.HEAD and raw.size == 3 + L * R.row_bytes(n)
    if n % 4:
        assert ((raw[3:].reshape(L, -1)[:, -1] >> (2 * (n % 4))) != 0).all()   # the pad bit pairs are garbage
    clean = R.write_codes(str(tmp_path / "b.bed"), codes, garbage_pad=False)
    g = np.array([-1, 0, 0, 1], dtype=np.int8)[codes]
    ref = synth.write_bed(str(tmp_path / "c"), g, missing=codes == 1)
    assert open(clean, "rb").read() == open(ref, "rb").read()


def test_neighbour_table_shape():
    for n, K in ((1, 3), (2, 4), (5, 8), (300, 256)):
        nbr = R.neighbour_table(n, K, seed=n)
        assert nbr.dtype == np.int32 and nbr.shape == (n, K) and nbr.min() >= -1 and nbr.max() < n
        assert not (nbr == np.arange(n)[:, None]).any()
        if n > 1:
            assert (nbr[1] == -1).all()
        for row in nbr:                                                        # -1 only as a tail
            k = int((row >= 0).sum())
            assert (row[:k] >= 0).all() and (row[k:] == -1).all()
    assert (R.neighbour_table(300, 256, seed=1)[::3] == -1).any() and (R.neighbour_table(300, 8, seed=1)[2] >= 0).all()


@pytest.mark.parametrize("n,L,K,k,min_votes", [(1, 3, 1, 1, 1), (5, 4, 8, 8, 1), (65, 17, 16, 5, 1), (65, 17, 16, 5, 3), (257, 9, 256, 1, 1),
                                               (257, 9, 256, 10, 2), (1025, 3, 8, 5, 1000)])
def test_sparse_imputation_is_the_host_restatement(n, L, K, k, min_votes):
    from eagleeverything_amd import r_api
    codes = R.codes_panel(n, L, seed=10 * n + K, rate=0.1, dense=0, full=1, empty=2)
    nbr = R.neighbour_table(n, K, seed=K)
    rows, counts = R.impute_knn_sparse(codes, nbr, k, min_votes)
    want_rows, want_counts = r_api.impute_knn_host(codes, nbr, k, min_votes)
    assert rows.dtype == want_rows.dtype and np.array_equal(rows, want_rows)
    assert counts.dtype == want_counts.dtype and np.array_equal(counts, want_counts)
    assert np.array_equal(counts.sum(axis=1), (codes == 1).sum(axis=1)) and counts[2].tolist() == [0, n]


def test_ld_neighbours_by_hand():
    p = R.ld_neighbours(40)
    assert p.shape == (40, 32) and p[0, :17].tolist() == list(range(1, 17)) + [-1] and p[20, :6].tolist() == [19, 21, 18, 22, 17, 23]
    assert (p[20] >= 0).all() and p[39, :3].tolist() == [38, 37, 36]
    for m in range(40):
        live = p[m][p[m] >= 0]
        assert sorted(live.tolist()) == [j for j in range(max(0, m - 16), min(40, m + 17)) if j != m]
    assert R.ld_neighbours(1).tolist() == [[-1] * 32]


def test_cluster_panel_makes_the_choice_of_voters_matter():
    from eagleeverything_amd import r_api
    n, L = 300, 40
    codes, full = R.cluster_panel(n, L, seed=1, rate=0.02)
    assert codes.shape == full.shape == (L, n) and not (full == 1).any() and 0.01 < (codes == 1).mean() < 0.03
    assert np.array_equal(codes[codes != 1], full[codes != 1])
    hidden = codes == 1
    part = R.ld_neighbours(L)
    rows, _ = r_api.impute_ldknn_host(codes, part, 16, 1, 4)                 # 16 voters: a founder has about 37 copies here
    far, _ = r_api.impute_ldknn_host(codes, np.full((L, 1), -1, dtype=np.int32), 16, 1, 1)      # no partner: the marker's own mean
    unpack = lambda r: np.stack([(r >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(L, -1)[:, :n]      # noqa: E731
    assert (unpack(rows)[hidden] == full[hidden]).mean() > 0.9 > 0.6 > (unpack(far)[hidden] == full[hidden]).mean()


def test_knn_row_is_a_row_of_the_host_restatement():
    from eagleeverything_amd import r_api
    n = 300
    d = R.dist_matrix(n, band=128)
    assert np.array_equal(d, R.dist_rows(np.arange(n), n)) and np.array_equal(d[[7, 250]], R.dist_rows([7, 250], n))
    for K in (1, 7, 256):
        want = r_api.knn_rows_host(d.view(np.int32), K)
        for i in (0, 1, 2, 3, 150, 299):
            assert np.array_equal(R.knn_row(d[i], i, K), want[i]), (K, i)
    assert np.array_equal(R.knn_row(d[1, :3], 1, 5), [0, 2, -1, -1, -1])      # row 1 holds one value: index order, then the -1 tail
    ibs0, hethet = R.ibs_matrices(n, band=64)
    dd = r_api.knn_distance(ibs0, hethet)
    assert dd.min() >= 0 and dd.max() < 376 + 64 and np.array_equal(np.diagonal(hethet), 30 + np.arange(n) % 32) and not np.diagonal(ibs0).any()
    want = r_api.knn_rows_host(dd, 40)
    for i in (0, 17, 299):
        a, h = R.ibs_rows([i], n)
        assert np.array_equal(a[0], ibs0[i]) and np.array_equal(h[0], hethet[i])
        row = (4 * a[0].astype(np.int64) + h[0, i] + np.diagonal(hethet) - 2 * h[0]).astype(np.int32)
        assert np.array_equal(row, dd[i]) and np.array_equal(R.knn_row(row, i, 40), want[i])


def test_dist_rows_hold_what_the_cases_need():
    n = 16385
    rows = R.sampled_rows(n)
    assert rows.size == 512 and np.unique(rows).size == 512 and rows[0] == 0 and rows[-1] == n - 1
    assert {4095, 4096, 4097, 4098, 4099, 16383, 16384}.issubset(set(rows.tolist()))
    assert np.array_equal(rows, R.sampled_rows(n)) and np.array_equal(R.sampled_rows(5), np.arange(5))
    d = R.dist_rows(rows, n)
    assert d.dtype == np.uint32 and d.shape == (512, n) and not (d == 0xffffffff).any()
    plain = d[rows % 4096 == 0]
    assert (plain == 0xfffffffe).mean() > 0.01 and (plain >= 0xffff0000).mean() > 0.3 and (plain < 4096).mean() > 0.6
    first = R.knn_row(plain[0], int(rows[rows % 4096 == 0][0]), 256)
    assert np.unique(plain[0][first]).size < 200                               # ties inside the list: the smaller j decides
    assert (d[rows % 4096 == 1] == 7).all() and (d[rows % 4096 == 2] >= 0xffff0000).all()
    rare = d[rows % 4096 == 3]
    assert 16 < (rare[0] != 0xfffffffe).sum() < 256                            # K = 256 runs into the no-overlap entries


def test_children_have_no_error_with_their_parents():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(4)
    par = rng.integers(-1, 2, size=(64, 4)).astype(np.int8)
    pairs = np.array([(0, 2), (0, 3), (1, 2), (1, 3)] * 3)
    kids = R.children(par, pairs, seed=1)
    g = np.concatenate((par, kids), axis=1)
    tab, _ = r_api.mendel_host(g, None, [(4 + c, s, d) for c, (s, d) in enumerate(pairs.tolist())])
    assert kids.shape == (64, 12) and set(np.unique(kids).tolist()) == {-1, 0, 1} and not tab[:, 5].any()
    best = r_api.parentage_host(g, None, np.arange(4, 16), [0, 1], [2, 3])
    assert np.array_equal(best[:, 0, :3], np.concatenate((pairs, np.zeros((12, 1), dtype=np.int64)), axis=1)) and (best[:, 1, 2] > 0).all()


def test_epistasis_host_sums_are_exact_integers():
    """epistasis_host forms its five pair sums as fp64 products while n max|y| < 2^53: the same integers as int64 products."""
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(11)
    n, L = 5000, 9
    G = rng.integers(-1, 2, size=(n, L)).astype(np.int64)
    y = rng.integers(-1000000, 1000001, n)
    y[0], y[-1] = 1000000, -1000000
    loci = np.array([0, 8, 3, 3])
    G2, B, B2 = G * G, G[:, loci], (G * G)[:, loci]
    want = np.stack([G.T @ B, G2.T @ B, G.T @ B2, G2.T @ B2, (G * y[:, None]).T @ B], axis=-1)
    got = r_api.epistasis_host(G.astype(np.int8), y, loci=loci)["mom"]
    assert got.dtype == np.int64 and np.array_equal(got, want)
