"""Line scores on the GPU: eagle_sample_scores / eagle_marker_scores (k_score_digits, k_line_scores_i8 on the tile engine of k_syrk_i8,
k_scores_finish) and the interface on top (r_api.Score, PCA(loadings=True), ProjectPCA, am.MarkerEffects, am.Predict).

Expected values are numpy's int64 products of tests/scores_truth.py, written from the definition of include/eagle_hip.h section
1b''''i; they share no code with the feature.  Every integer comparison is array_equal / tobytes; every fp comparison uses a bound
computed here from the returned scales plus the standard bound of the comparison's own fp64 sums."""
import functools
import os

import numpy as np
import pytest

from scores_truth import EDGES, EPS, W30, dot_bound, edge_panel, edge_weights, k_splits, np_scores


def ingest(tmp, M8):
    from eagleeverything_amd import synth
    os.makedirs(str(tmp), exist_ok=True)
    return synth.write_geno_pair(str(tmp), np.ascontiguousarray(M8.T))


@functools.lru_cache(maxsize=None)
def edge_case(by_marker, T):
    """(image, weights, truth) of the edge panel's M file (by_marker False) or Mt file for T columns; read-only, computed once."""
    M8 = edge_panel()
    G8 = np.ascontiguousarray(M8.T) if by_marker else M8
    w = edge_weights(T, G8.shape[1], seed=100 * T + by_marker)
    truth = np_scores(G8, w)
    for a in (G8, w, truth):
        a.setflags(write=False)
    return G8, w, truth


def call(rcpp_api, geno, by_marker, w, **kw):
    fn, path = (rcpp_api.marker_scores, geno["asciifileMt"]) if by_marker else (rcpp_api.sample_scores, geno["asciifileM"])
    return fn(path, geno["dim_of_ascii_M"], w, **kw)


# ------------------------------------------------------------------------------------------------ 1. fixtures against numpy
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["genoDemo_150x4998", "synth_203x1531"])
def test_gpu_scores_on_fixtures(golden, tmp_path, case):
    from eagleeverything_amd import rcpp_api
    M8 = golden(case)["M8"]
    n, L = M8.shape
    rng = np.random.default_rng(L)
    w, v = rng.integers(-W30, W30 + 1, (3, L)), rng.integers(-W30, W30 + 1, (3, n))
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    S = rcpp_api.sample_scores(geno["asciifileM"], (n, L), w)
    assert S.dtype == np.int64 and S.shape == (n, 3)
    assert S[3, 1] == sum(int(w[1, m]) * int(M8[3, m]) for m in range(L))                 # the definition on one element
    assert np.array_equal(S, np_scores(M8, w))
    U = rcpp_api.marker_scores(geno["asciifileMt"], (n, L), v)
    assert U.dtype == np.int64 and U.shape == (L, 3) and np.array_equal(U, np_scores(M8.T, v))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 2. tile, split and digit edges
@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5, 64])
def test_gpu_scores_tile_split_and_digit_edges(tmp_path, T):
    from eagleeverything_amd import r_api, rcpp_api
    M8 = edge_panel()
    n, L = M8.shape
    assert (n, L) == (1003, 5000) and n % 128 and L % 128 and n > 768
    # 5,000 characters are 40 K stages of 128 bytes: two splits of 20 under the 16-stage rule, so a lost or doubled split shows; the
    # 1,003 characters of an Mt line are 8 stages, one split
    assert k_splits(L) == (40, 2) and k_splits(n) == (8, 1)
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    for by_marker in (False, True):
        G8, w, truth = edge_case(by_marker, T)
        assert all(int(x) in w[0] for x in EDGES) and np.abs(w).max() == W30
        planes = r_api.score_digits_host(w)
        if T >= 5:
            assert not planes[1:, 1].any() and planes[0, 1].any()                        # one plane
            assert not planes[0, 2].any() and planes[1:, 2].any()                        # plane 0 empty
            assert not w[3].any()                                                        # a zero column
        got = call(rcpp_api, geno, by_marker, w)
        assert got.dtype == np.int64 and got.shape == (G8.shape[0], T)
        assert np.array_equal(got, truth)
        if T >= 5:
            assert not got[:, 3].any()
    rcpp_api.drop_cache()


@pytest.mark.gpu
def test_gpu_scores_units_ones_and_column_split(tmp_path):
    from eagleeverything_amd import rcpp_api
    M8 = edge_panel()
    n, L = M8.shape
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    dims = (n, L)
    # unit columns: e_m returns marker m's genotype column, e_i individual i's row -- a wrong element is named
    ms = [0, 1, 127, 128, 255, 256, 2559, 2560, 4095, 4096, 4999]
    E = np.zeros((len(ms), L), dtype=np.int64)
    E[np.arange(len(ms)), ms] = 1
    got = rcpp_api.sample_scores(geno["asciifileM"], dims, E)
    bad = np.argwhere(got != M8[:, ms])
    assert bad.size == 0, "individual %d, marker %d" % (bad[0, 0], ms[bad[0, 1]])
    ids = [0, 1, 127, 128, 255, 256, 511, 512, 767, 768, 1002]
    E = np.zeros((len(ids), n), dtype=np.int64)
    E[np.arange(len(ids)), ids] = 1
    got = rcpp_api.marker_scores(geno["asciifileMt"], dims, E)
    bad = np.argwhere(got != M8[ids].T)
    assert bad.size == 0, "marker %d, individual %d" % (bad[0, 0], ids[bad[0, 1]])
    # all-ones weights are n2 - n0 of the counting pass over the same images
    cs = rcpp_api.sample_counts(geno["asciifileM"], dims).astype(np.int64)
    assert np.array_equal(rcpp_api.sample_scores(geno["asciifileM"], dims, np.ones(L, dtype=np.int8))[:, 0], cs[:, 2] - cs[:, 0])
    cm = rcpp_api.marker_counts(geno["asciifileMt"], dims).astype(np.int64)
    assert np.array_equal(rcpp_api.marker_scores(geno["asciifileMt"], dims, np.ones(n, dtype=np.uint16))[:, 0], cm[:, 2] - cm[:, 0])
    assert not rcpp_api.sample_scores(geno["asciifileM"], dims, np.zeros((2, L), dtype=np.int32)).any()     # no plane at all
    # 65 columns through the wrapper's split equal the same columns in two calls
    w = np.random.default_rng(65).integers(-W30, W30 + 1, (65, L))
    all65 = rcpp_api.sample_scores(geno["asciifileM"], dims, w)
    assert all65.shape == (n, 65)
    assert np.array_equal(all65[:, :64], rcpp_api.sample_scores(geno["asciifileM"], dims, w[:64]))
    assert np.array_equal(all65[:, 64:], rcpp_api.sample_scores(geno["asciifileM"], dims, w[64:]))
    assert np.array_equal(all65[:, 64], np_scores(M8, w[64])[:, 0])
    rcpp_api.drop_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("n,L", [(1, 1), (1, 129), (257, 1)])
def test_gpu_scores_tiny_files(tmp_path, n, L):
    from eagleeverything_amd import rcpp_api
    rng = np.random.default_rng(n * 1000 + L)
    M8 = rng.integers(-1, 2, (n, L)).astype(np.int8)
    M8[0, 0] = -1
    w, v = edge_weights(2, L, seed=1), edge_weights(2, n, seed=2)
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    assert np.array_equal(rcpp_api.sample_scores(geno["asciifileM"], (n, L), w), np_scores(M8, w))
    assert np.array_equal(rcpp_api.marker_scores(geno["asciifileMt"], (n, L), v), np_scores(M8.T, v))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 3. streamed equals resident
@pytest.mark.gpu
def test_gpu_scores_streamed_equals_resident(tmp_path, monkeypatch):
    from eagleeverything_amd import r_api, rcpp_api
    M8 = edge_panel()
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
    res = {}
    for by_marker in (False, True):
        _, w, truth = edge_case(by_marker, 5)
        res[by_marker] = call(rcpp_api, geno, by_marker, w)
        assert np.array_equal(res[by_marker], truth)
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.001")          # bands of 256 lines, from the sidecar
    assert os.path.exists(geno["asciifileM"] + ".e2b") and os.path.exists(geno["asciifileMt"] + ".e2b")
    for by_marker in (False, True):
        assert call(rcpp_api, geno, by_marker, edge_case(by_marker, 5)[1]).tobytes() == res[by_marker].tobytes()
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")                      # the same bands from the text
    for by_marker in (False, True):
        assert call(rcpp_api, geno, by_marker, edge_case(by_marker, 5)[1]).tobytes() == res[by_marker].tobytes()
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 4. a VIEW
@pytest.mark.gpu
def test_gpu_scores_of_a_view(tmp_path):
    from eagleeverything_amd import am, rcpp_api
    M8 = edge_panel()
    n, L = M8.shape
    drop = np.array([1, 2, 256, 257, 500, 768, 1003], dtype=np.int64)  # 1-based; across tile edges, the first and the last individual
    kept = np.setdiff1d(np.arange(n), drop - 1)
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    sub = am.reshape_geno(geno, drop, view=True)
    nk = n - drop.size
    assert list(sub["dim_of_ascii_M"]) == [nk, L]
    v = edge_weights(5, nk, seed=41)
    assert np.array_equal(rcpp_api.marker_scores(sub["asciifileMt"], (nk, L), v), np_scores(M8[kept].T, v))
    w = edge_case(False, 5)[1]
    assert np.array_equal(rcpp_api.sample_scores(sub["asciifileM"], (nk, L), w), np_scores(M8[kept], w))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 5. the cached images are untouched
@pytest.mark.gpu
def test_gpu_scores_leave_the_cached_operand_alone(golden, tmp_path):
    from eagleeverything_amd import rcpp_api
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    w = np.random.default_rng(3).integers(-W30, W30 + 1, (3, L))
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    before = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L))     # makes the cached fp4 image
    assert np.array_equal(before, M8.astype(np.float64) @ M8.astype(np.float64).T)
    S = rcpp_api.sample_scores(geno["asciifileM"], (n, L), w)
    after = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L))
    assert after.tobytes() == before.tobytes() and np.array_equal(S, np_scores(M8, w))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 6. Score
@pytest.mark.gpu
def test_gpu_score_within_its_bound(golden, tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    rng = np.random.default_rng(6)
    W = rng.standard_normal((L, 3)) * np.array([1.0, 1e-6, 250.0])[None, :]
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    Mf = M8.astype(np.float64)
    sc = r_api.Score(geno, W)
    assert sc["S"].dtype == np.int64 and sc["score"].shape == (n, 3) and sc["wq"].dtype == np.int32
    assert np.array_equal(sc["S"], np_scores(M8, sc["wq"].T))
    for t in range(3):
        bound = 0.5 * L / sc["scale"][t]
        assert sc["bound"][t] == bound
        err = np.abs(sc["score"][:, t] - Mf @ W[:, t]).max()
        print("Score column %d: error %.3e, bound %.3e" % (t, err, bound))
        assert err <= bound + dot_bound(Mf, W[:, t])
    one = r_api.Score(geno, W[:, 0])
    assert one["score"].shape == (n, 1) and np.array_equal(one["S"][:, 0], sc["S"][:, 0])
    inc = np.arange(L) % 3 == 1
    si = r_api.Score(geno, W, include=inc)
    assert not si["wq"][~inc].any() and np.array_equal(si["S"], np_scores(M8[:, inc], si["wq"][inc].T))
    assert np.array_equal(si["bound"], 0.5 * inc.sum() / si["scale"])
    for t in range(3):
        assert np.abs(si["score"][:, t] - Mf[:, inc] @ W[inc, t]).max() <= si["bound"][t] + dot_bound(Mf[:, inc], W[inc, t])
    sd = r_api.Score(geno, W, dosage=True)                                               # the 0 / 1 / 2 allele count
    assert np.array_equal(sd["S"], np_scores(M8.astype(np.int64) + 1, sd["wq"].T))
    for t in range(3):
        assert np.abs(sd["score"][:, t] - (Mf + 1.0) @ W[:, t]).max() <= sd["bound"][t] + dot_bound(Mf + 1.0, W[:, t])
        assert sd["bound"][t] == 1.0 * L / sd["scale"][t]
    with pytest.raises(ValueError):
        r_api.Score(geno, W[:-1])
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 7. PCA loadings and projection
@pytest.mark.gpu
def test_gpu_pca_loadings_project_any_panel(golden, tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    R = np.array([i for i in range(n) if i % 5 != 4])
    k = 4
    rcpp_api.drop_cache()
    geno = ingest(tmp_path / "a", M8)
    plain = r_api.PCA(geno, k=k, reference=R)
    pca = r_api.PCA(geno, k=k, reference=R, loadings=True)
    assert set(pca) - set(plain) == {"loadings", "offset", "loadings_bound"}
    for key in ("values", "pcs", "explained", "reference"):
        assert np.asarray(pca[key]).tobytes() == np.asarray(plain[key]).tobytes()         # what it returned before
    assert pca["grm"]["G"].tobytes() == plain["grm"]["G"].tobytes()
    used, G = pca["grm"]["used"], pca["grm"]["G"]
    proj = r_api.ProjectPCA(pca, geno)
    assert proj.shape == (n, k) and proj.dtype == np.float64
    _, sc = r_api.quantise_weights(pca["loadings"])
    for a in range(k):
        fp = dot_bound(G[:, R], np.abs(pca["pcs"][R][:, a])) / pca["values"][a] + dot_bound(np.ones((1, L)), np.abs(pca["loadings"][:, a]))
        bound = 0.5 * L / sc[a] + 2.0 * used.sum() * pca["loadings_bound"][a] + 4.0 * fp
        err = np.abs(proj[:, a] - pca["pcs"][:, a])
        print("component %d: members %.3e, others %.3e, bound %.3e" % (a, err[R].max(), np.delete(err, R).max(), bound))
        assert err.max() <= bound and bound < 1e-4 * np.abs(pca["pcs"][:, a]).max()
    # permuted and duplicated rows as a second panel: exact integer sums, so the very same coordinates
    pick = np.random.default_rng(7).integers(0, n, 300)
    pick[:5] = (0, 0, n - 1, 4, 4)
    geno2 = ingest(tmp_path / "b", M8[pick])
    proj2 = r_api.ProjectPCA(pca, geno2)
    assert proj2.shape == (300, k) and proj2.tobytes() == proj[pick].tobytes()
    with pytest.raises(ValueError):
        r_api.ProjectPCA(pca, ingest(tmp_path / "c", M8[:, :-1]))
    with pytest.raises(ValueError):
        r_api.ProjectPCA(plain, geno)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 8. marker effects and prediction
@pytest.mark.gpu
def test_gpu_marker_effects_and_predict(golden, tmp_path):
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    M8 = golden("genoDemo_150x4998")["M8"]
    n, L = M8.shape
    y, _ = synth.trait(np.ascontiguousarray(M8.T))
    na = np.random.default_rng(8).choice(n, 20, replace=False)
    y = y.copy()
    y[na] = np.nan
    trained = np.setdiff1d(np.arange(n), na)
    X = np.ones((n, 1))
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    res = am.AM(y, X, geno, maxit=3)
    assert sorted(int(i) - 1 for i in res["indxNA"]) == sorted(na.tolist())
    eff = am.MarkerEffects(res, y, X, geno)
    nt = trained.size
    assert nt == 130 and eff["u"].shape == (L,) and eff["Py"].shape == (nt,) and eff["loci"] == [int(j) for j in res["selected_loci"]]
    assert eff["beta"].shape == (1 + len(eff["loci"]),) and eff["ve"] >= 0 and eff["vg"] >= 0
    d = eff["weights"] - eff["u"]
    assert np.count_nonzero(d) <= len(eff["loci"]) and all(d[j - 1] == (eff["u"][j - 1] + eff["beta"][1 + i]) - eff["u"][j - 1]
                                                           for i, j in enumerate(eff["loci"]))
    view = am.reshape_geno(geno, res["indxNA"], view=True)
    MMt = rcpp_api.calculateMMt_rcpp(view["asciifileM"], 8.0, 1, np.nan, (nt, L))
    assert np.array_equal(MMt, M8[trained].astype(np.float64) @ M8[trained].astype(np.float64).T)
    c = 1.0 / MMt.max()
    assert eff["c"] == c
    pv = am.Predict(eff, view)
    ref = eff["vg"] * c * (MMt @ eff["Py"])
    fp = 2.0 * eff["vg"] * c * dot_bound(MMt, eff["Py"]) + 8.0 * EPS * np.abs(ref).max()
    tol = L * eff["bound"] + pv["bound"][0] + fp
    err = np.abs(pv["polygenic"] - ref).max()
    print("polygenic: error %.3e, tolerance %.3e (scale %.3e)" % (err, tol, np.abs(ref).max()))
    assert err <= tol and (tol < 1e-3 * np.abs(ref).max() or eff["vg"] == 0)          # the tolerance says something: three digits
    K = MMt * c
    K.flat[:: nt + 1] += 0.95
    tol2 = tol + 2.0 * eff["vg"] * dot_bound(K, eff["Py"]) + 8.0 * EPS * np.abs(eff["ghat"]).max()
    assert np.abs(pv["polygenic"] + 0.95 * eff["vg"] * eff["Py"] - eff["ghat"]).max() <= tol2
    full = am.Predict(eff, geno, X=X)
    for key in ("polygenic", "genetic", "yhat"):
        assert full[key].shape == (n,) and np.all(np.isfinite(full[key]))
    assert full["polygenic"][trained].tobytes() == pv["polygenic"].tobytes()             # exact sums: an individual's own genotypes alone
    assert full["genetic"][trained].tobytes() == pv["genetic"].tobytes()
    assert np.array_equal(full["yhat"], X @ eff["beta"][:1] + full["genetic"])
    assert np.array_equal(r_api.Predict(eff, geno)["genetic"], full["genetic"])
    rcpp_api.drop_cache()
