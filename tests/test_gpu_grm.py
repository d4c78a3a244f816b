"""GRM and PCA on the GPU: eagle_weighted_gram (k_scale_cols_i8, k_gram_i8ab on the tile engine of k_syrk_i8, k_wgram_finish) and the
r_api interface on top (GRM, PCA, am.add_pcs into AM).

Expected values are the numpy restatements of tests/test_grm_host.py, written from the definition of include/eagle_hip.h section
1b'''': Q = (G * q) @ G.T in int64, the directly centred and scaled panel for the relationship matrix and its components.  They share
no code with the feature.  Every integer comparison is array_equal."""
import functools
import os

import numpy as np
import pytest

from test_grm_host import QMAX, assert_pca_properties, counts_of, np_wgram, structured_truth

DIGIT_EDGES = (0, 1, 127, 128, 129, 16383, 16384, 16385, QMAX)


def ingest(tmp, M8):
    from eagleeverything_amd import synth
    return synth.write_geno_pair(str(tmp), np.ascontiguousarray(M8.T))


@functools.lru_cache(maxsize=None)
def edge_panel():
    """1,003 x 5,000 (n crosses the 256, 512 and 768 tile edges, L is no multiple of 128 or 256), weights that cycle through the edges
    of the three base-128 digits and then random ones.  -> (M8, q, Q), read-only."""
    from eagleeverything_amd import synth
    M8 = np.ascontiguousarray(synth.genotypes_marker_major(1003, 5000, seed=1234).T)
    L = M8.shape[1]
    q = np.random.default_rng(5).integers(0, QMAX + 1, L).astype(np.uint32)
    q[:2700] = np.tile(np.array(DIGIT_EDGES, dtype=np.uint32), 300)
    Q = np_wgram(M8, q)
    for a in (M8, q, Q):
        a.setflags(write=False)
    return M8, q, Q


# ------------------------------------------------------------------------------------------------ 1. fixtures against numpy
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["genoDemo_150x4998", "synth_203x1531"])
def test_gpu_weighted_gram_on_fixtures(golden, tmp_path, case):
    from eagleeverything_amd import rcpp_api
    M8 = golden(case)["M8"]
    n, L = M8.shape
    q = np.random.default_rng(L).integers(0, QMAX + 1, L)
    truth = np_wgram(M8, q)
    assert truth[3, 77] == sum(int(q[m]) * int(M8[3, m]) * int(M8[77, m]) for m in range(L))      # the restatement on one pair
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    Q = rcpp_api.weighted_gram(geno["asciifileM"], (n, L), q)
    assert Q.dtype == np.int64 and Q.shape == (n, n) and np.array_equal(Q, Q.T)
    assert np.array_equal(Q, truth)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 2. tile edges and digit edges
@pytest.mark.gpu
def test_gpu_weighted_gram_tile_and_digit_edges(tmp_path):
    from eagleeverything_amd import rcpp_api
    M8, q, truth = edge_panel()
    n, L = M8.shape
    assert all(int(v) in q for v in DIGIT_EDGES) and q.max() == QMAX
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    fM = geno["asciifileM"]
    Q = rcpp_api.weighted_gram(fM, (n, L), q)
    assert Q.dtype == np.int64 and Q.shape == (n, n) and np.array_equal(Q, Q.T) and np.array_equal(Q, truth)
    mmt = rcpp_api.calculateMMt_rcpp(fM, 8.0, 2, np.nan, (n, L))
    assert np.array_equal(mmt, np_wgram(M8, np.ones(L, dtype=np.int64)))
    ones = rcpp_api.weighted_gram(fM, (n, L), np.ones(L, dtype=np.uint32))                         # one plane: MM^T itself
    assert np.array_equal(ones, mmt.astype(np.int64)) and np.array_equal(ones.astype(np.float64), mmt)
    assert not rcpp_api.weighted_gram(fM, (n, L), np.zeros(L, dtype=np.uint32)).any()              # no plane
    mid = rcpp_api.weighted_gram(fM, (n, L), np.full(L, 128))                                      # the middle plane alone
    assert np.array_equal(mid, 128 * ones)
    subset = np.arange(L) % 5 == 2                                                                 # weights in {0, 1}: a marker subset
    assert np.array_equal(rcpp_api.weighted_gram(fM, (n, L), subset), np_wgram(M8[:, subset], np.ones(subset.sum(), dtype=np.int64)))
    with pytest.raises(ValueError):
        rcpp_api.weighted_gram(fM, (n, L), q[:-1])
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 3. streamed equals resident
@pytest.mark.gpu
def test_gpu_weighted_gram_streamed_equals_resident(tmp_path, monkeypatch):
    from eagleeverything_amd import r_api, rcpp_api
    M8, q, truth = edge_panel()
    n, L = M8.shape
    rcpp_api.drop_cache()
    d = tmp_path / "p"
    d.mkdir()
    table = np.full((n, 2 * L), ord(" "), dtype=np.uint8)
    table[:, 0::2] = M8 + 1 + ord("0")
    table[:, -1] = ord("\n")
    (d / "table.txt").write_bytes(table.tobytes())
    geno = r_api.ReadMarker(str(d / "table.txt"), type="text", AA=0, AB=1, BB=2, outdir=str(d))    # writes the sidecars
    assert geno is not None and list(geno["dim_of_ascii_M"]) == [n, L]
    res = rcpp_api.weighted_gram(geno["asciifileM"], (n, L), q)
    assert np.array_equal(res, truth)
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.001")          # windows of 256 markers, from the sidecar
    assert os.path.exists(geno["asciifileM"] + ".e2b")
    got = rcpp_api.weighted_gram(geno["asciifileM"], (n, L), q)
    assert got.tobytes() == res.tobytes()
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")                      # the same windows from the text
    got = rcpp_api.weighted_gram(geno["asciifileM"], (n, L), q)
    assert got.tobytes() == res.tobytes()
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 4. the cached images are untouched
@pytest.mark.gpu
def test_gpu_weighted_gram_leaves_the_cached_operand_alone(golden, tmp_path):
    from eagleeverything_amd import rcpp_api
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    q = np.random.default_rng(3).integers(0, QMAX + 1, L)
    truth = M8.astype(np.float64) @ M8.astype(np.float64).T
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    before = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L))     # makes the cached fp4 image
    assert np.array_equal(before, truth)
    Q = rcpp_api.weighted_gram(geno["asciifileM"], (n, L), q)
    after = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L))
    assert after.tobytes() == before.tobytes() and np.array_equal(Q, np_wgram(M8, q))
    rcpp_api.drop_cache()                                                               # and in the other order, on a fresh file
    Q2 = rcpp_api.weighted_gram(geno["asciifileM"], (n, L), q)
    assert Q2.tobytes() == Q.tobytes()
    assert rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L)).tobytes() == before.tobytes()
    assert rcpp_api.weighted_gram(geno["asciifileM"], (n, L), q).tobytes() == Q.tobytes()
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 5. small edges
@pytest.mark.gpu
@pytest.mark.parametrize("n,L", [(1, 1), (2, 33), (37, 33), (37, 300), (257, 129)])
def test_gpu_weighted_gram_small_edges(tmp_path, n, L):
    from eagleeverything_amd import rcpp_api
    rng = np.random.default_rng(100 * n + L)
    M8 = rng.integers(-1, 2, size=(n, L)).astype(np.int8)
    q = rng.integers(0, QMAX + 1, L).astype(np.uint32)
    q[L - 1] = QMAX                                                    # the last marker, beside the column padding
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    Q = rcpp_api.weighted_gram(geno["asciifileM"], (n, L), q)
    assert Q.dtype == np.int64 and Q.shape == (n, n) and np.array_equal(Q, np_wgram(M8, q))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 6. a VIEW
@pytest.mark.gpu
def test_gpu_weighted_gram_of_a_view(tmp_path):
    from eagleeverything_amd import am, rcpp_api
    M8, q, _ = edge_panel()
    n, L = M8.shape
    drop = np.array([1, 2, 256, 257, 500, 768, 1003], dtype=np.int64)  # 1-based; across tile edges, the first and the last individual
    kept = np.setdiff1d(np.arange(n), drop - 1)
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    sub = am.reshape_geno(geno, drop, view=True)
    assert list(sub["dim_of_ascii_M"]) == [n - drop.size, L]
    Q = rcpp_api.weighted_gram(sub["asciifileM"], (n - drop.size, L), q)
    assert np.array_equal(Q, np_wgram(M8[kept], q))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 7. end to end
@pytest.mark.gpu
def test_gpu_pca_of_three_populations_into_am(tmp_path):
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    M8, labels, R, G_t, lam_t, pcs_t = structured_truth()              # asserts the restatement's own figures first
    n, L = M8.shape
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    pca = r_api.PCA(geno, k=2, reference=R)
    grm = pca["grm"]
    n0, n1, n2 = counts_of(M8, R)
    assert np.array_equal(grm["n0"], n0) and np.array_equal(grm["n1"], n1) and np.array_equal(grm["n2"], n2)   # counted over R alone
    assert grm["used"].all() and grm["q"].max() == QMAX and 0 < grm["weight_rel_error"] < 1e-5
    assert grm["Q"].dtype == np.int64 and np.array_equal(grm["Q"], np_wgram(M8, grm["q"]))
    # the same double-centring in the restatement's order, from the directly centred panel with the weights q / scale
    mu = M8[R].astype(np.float64).mean(axis=0)
    Z = (M8 - mu[None, :]) * np.sqrt(grm["q"] / grm["scale"])[None, :]
    G_q = Z @ Z.T / L
    assert np.max(np.abs(grm["G"] - G_q)) <= 1e-12 * np.max(np.abs(G_q))
    assert_pca_properties(pca, labels, R, G_t, pcs_t, 2)
    assert np.allclose(pca["values"], lam_t[:2], rtol=1e-5) and np.array_equal(pca["reference"], R)
    # the same matrix from the whole file in one call and from one marker subset per "chromosome"
    chrom = np.arange(L) * 3 // L
    parts = [r_api.GRM(geno, reference=R, include=chrom == c, stats=grm) for c in range(3)]
    for c, part in enumerate(parts):
        assert np.array_equal(part["used"], chrom == c) and np.array_equal(part["Q"], np_wgram(M8, part["q"]))
    y, _ = synth.trait(np.ascontiguousarray(M8.T), nqtl=3, beta=1.5, seed=5)
    X = np.ones((n, 1))
    res = am.AM(y, am.add_pcs(X, pca), geno, maxit=3)
    assert len(res["selected_loci"]) >= 1
    rcpp_api.drop_cache()
