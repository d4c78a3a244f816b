"""CPU: the host side of GRM / PCA -- r_api.grm_weights, grm_from_gram, PCA(grm=), am.add_pcs, the ValueErrors of
rcpp_api.weighted_gram -- against restatements written here from the definitions of include/eagle_hip.h section 1b'''' and the
docstrings: a scalar loop for the weights (bit for bit), the direct centre-scale-multiply definition and fractions.Fraction for the
matrix, a numpy PCA of the directly centred panel for the components.  They share no code with the feature.  No device work; the
restatements and the three-population panel are what tests/test_gpu_grm.py compares the device results with."""
import functools
from fractions import Fraction

import numpy as np
import pytest

QMAX = 2097151


# ---- restatements ----
def np_wgram(M8, q):
    """Q = (G * q) @ G.T -> int64, for an n x L matrix of -1 / 0 / +1.  Every partial sum is an integer below L * max(q) in
    magnitude: while that is below 2^53 the float64 product (BLAS) is exact in any order; a small panel is multiplied in int64."""
    q = np.asarray(q, dtype=np.int64)
    n, L = np.shape(M8)
    assert q.shape == (L,) and L * int(q.max(initial=0)) < 2 ** 53
    if n <= 40:
        G = np.asarray(M8, dtype=np.int64)
        return (G * q[None, :]) @ G.T
    G = np.asarray(M8, dtype=np.float64)
    return ((G * q.astype(np.float64)[None, :]) @ G.T).astype(np.int64)


def counts_of(M8, rows=None):
    """(n0, n1, n2) per marker over the individuals `rows` (default all) of an n x L matrix of -1 / 0 / +1."""
    G = np.asarray(M8) if rows is None else np.asarray(M8)[rows]
    return tuple(np.sum(G == v, axis=0).astype(np.int64) for v in (-1, 0, 1))


def py_weights(n0, n1, n2, method="standardized", maf=0.0, include=None):
    """grm_weights as a scalar loop over the markers, Python ints and floats in the documented order."""
    L = len(n0)
    w, used = [0.0] * L, [False] * L
    for m in range(L):
        N = int(n0[m]) + int(n1[m]) + int(n2[m])
        c = 2 * int(n2[m]) + int(n1[m])
        den = c * (2 * N - c)
        used[m] = den > 0 and float(min(c, 2 * N - c)) >= maf * float(2 * N) and (include is None or bool(include[m]))
        if used[m]:
            w[m] = ((2.0 * float(N)) * float(N)) / float(den)
    if not any(used):
        return np.zeros(L, dtype=np.uint32), 1.0, np.array(used, dtype=bool), w
    if method == "vanraden1":
        return np.array([1 if u else 0 for u in used], dtype=np.uint32), 1.0, np.array(used, dtype=bool), w
    scale = 2097151.0 / max(w[m] for m in range(L) if used[m])
    q = [int(np.rint(w[m] * scale)) if used[m] else 0 for m in range(L)]
    return np.array(q, dtype=np.uint32), scale, np.array(used, dtype=bool), w


def direct_grm(M8, q, scale, used, method, R):
    """The definition: centre every marker at its mean over R, scale, multiply (fp64)."""
    G = np.asarray(M8, dtype=np.float64)
    mu = G[R].mean(axis=0)
    Z = (G - mu[None, :]) * np.sqrt(np.asarray(q, dtype=np.float64))[None, :]
    Gc = Z @ Z.T
    if method == "standardized":
        return Gc / (scale * used.sum())
    p = (mu[used] + 1.0) / 2.0
    return Gc / np.sum(2.0 * p * (1.0 - p))


def structured_panel():
    """303 x 3,000, three populations (label i % 3), Balding-Nichols at Fst 0.05 around ancestral frequencies U(0.1, 0.9); rows
    300 .. 302 are copies of rows 0 .. 2.  -> (M8 n x L int8 in -1 / 0 / +1, labels, reference = arange(300))."""
    rng = np.random.default_rng(2024)
    n, L, fst = 303, 3000, 0.05
    anc = rng.uniform(0.1, 0.9, L)
    a, b = anc * (1 - fst) / fst, (1 - anc) * (1 - fst) / fst
    freq = np.stack([rng.beta(a, b) for _ in range(3)], axis=0)            # 3 x L
    labels = np.arange(n) % 3
    M8 = (rng.binomial(2, freq[labels]) - 1).astype(np.int8)
    M8[300:303] = M8[0:3]
    return M8, labels, np.arange(300, dtype=np.int64)


def np_pca(M8, R, k, maf=0.0):
    """The restatement: exact fp64 weights 1 / (2 p (1 - p)) from the allele frequencies over R (no quantisation), the directly
    centred and scaled panel, eigh of its Gram matrix over R, projection of every row.  -> G (n x n), values (k), pcs (n x k)."""
    G8 = np.asarray(M8, dtype=np.float64)
    p = (G8[R].mean(axis=0) + 1.0) / 2.0
    use = (p > 0) & (p < 1) & (np.minimum(p, 1 - p) >= maf)
    Z = (G8[:, use] + 1.0 - 2.0 * p[use][None, :]) / np.sqrt(2.0 * p[use] * (1.0 - p[use]))[None, :]
    G = Z @ Z.T / use.sum()
    lam, U = np.linalg.eigh(G[np.ix_(R, R)])
    lam, U = lam[::-1][:k], U[:, ::-1][:, :k]
    return G, lam, (G[:, R] @ U) / lam[None, :], U


def misclassified(pcs, labels, R):
    """Individuals whose nearest population centroid (centroids over R, first two components) is not their own; the largest
    within-population distance to the centroid and the smallest distance between two centroids."""
    P = pcs[:, :2]
    cen = np.stack([P[R][labels[R] == c].mean(axis=0) for c in range(3)], axis=0)
    d = np.linalg.norm(P[:, None, :] - cen[None, :, :], axis=2)
    within = d[np.arange(P.shape[0]), labels].max()
    between = min(np.linalg.norm(cen[a] - cen[b]) for a in range(3) for b in range(a))
    return int(np.sum(np.argmin(d, axis=1) != labels)), float(within), float(between)


@functools.lru_cache(maxsize=None)
def structured_truth():
    """The panel and its restatement, asserted on the restatement alone (the figures of the issue this feature answers); read-only."""
    M8, labels, R = structured_panel()
    G, lam, pcs, U = np_pca(M8, R, 3)
    assert abs(lam[0] - 11.2) < 0.15 and abs(lam[1] - 10.6) < 0.15 and abs(lam[2] - 1.7) < 0.1, lam
    bad, within, between = misclassified(pcs, labels, R)
    assert bad == 0 and within <= 0.020 and between >= 0.14, (bad, within, between)
    # reference rows reproduce their eigenvector entries and the duplicates land on their twins (measured: 3e-16 and below; the bound
    # is that of a 300-term fp64 dot product of unit vectors, divided by an eigenvalue above 10)
    assert np.max(np.abs(pcs[R] - U)) <= 1e-14 and np.max(np.abs(pcs[300:303] - pcs[0:3])) <= 1e-14
    for a in (M8, labels, R, G, lam, pcs):
        a.setflags(write=False)
    return M8, labels, R, G, lam, pcs


# ---- grm_weights ----
@pytest.mark.parametrize("case", ["genoDemo_150x4998", "synth_203x1531"])
def test_grm_weights_bit_for_bit(golden, case):
    from eagleeverything_amd import r_api
    M8 = golden(case)["M8"].copy()
    M8[:, 5] = 1                                                           # monomorphic markers: all BB, all AB, all AA
    M8[:, 6] = 0
    M8[:, 7] = -1
    M8[:, 8] = -1
    M8[0, 8] = 0                                                           # a single copy of the rare allele: the largest weight
    n, L = M8.shape
    n0, n1, n2 = counts_of(M8)
    include = np.arange(L) % 7 != 3
    for kw in ({}, {"maf": 0.05}, {"maf": 0.2, "include": include}, {"include": include}):
        q, scale, used = r_api.grm_weights(n0, n1, n2, **kw)
        tq, tscale, tused, w = py_weights(n0, n1, n2, **kw)
        assert q.dtype == np.uint32 and q.shape == (L,) and used.dtype == bool and isinstance(scale, float)
        assert np.array_equal(used, tused) and np.array_equal(q, tq) and scale == tscale
        assert q.max() == QMAX and np.all(q[~used] == 0) and not used[5] and not used[7]
        assert used[6] == bool(kw.get("include", np.ones(L, bool))[6])        # all heterozygous: p = 0.5, polymorphic
        if "maf" in kw:
            mafs = np.minimum(2 * n2 + n1, 2 * n0 + n1) / (2.0 * n)
            assert not used[mafs < kw["maf"]].any() and (mafs < kw["maf"]).any() and not used[8]
        else:
            assert used[8] == bool(kw.get("include", np.ones(L, bool))[8])
        if "include" in kw:
            assert not used[~include].any()
        # the documented error bound of a weight, and that the worst one is met by the marker nearest p = 0.5
        wa = np.array(w)[used]
        rel = np.abs(q[used] / scale - wa) / wa
        assert np.all(rel <= wa.max() / (wa * (2.0 ** 22 - 2)) * (1 + 1e-12))
    q, scale, used = r_api.grm_weights(n0, n1, n2, method="vanraden1", maf=0.05)
    tq, tscale, tused, _ = py_weights(n0, n1, n2, method="vanraden1", maf=0.05)
    assert scale == 1.0 and np.array_equal(q, tq) and np.array_equal(used, tused) and set(np.unique(q).tolist()) == {0, 1}
    assert np.array_equal(q == 1, used)
    q, scale, used = r_api.grm_weights(n0[5:6], n1[5:6], n2[5:6])          # nothing usable
    assert q.tolist() == [0] and scale == 1.0 and used.tolist() == [False]
    with pytest.raises(ValueError):
        r_api.grm_weights(n0, n1, n2, method="gcta")
    with pytest.raises(ValueError):
        r_api.grm_weights(n0, n1, n2, include=include[:-1])


def test_grm_weight_error_on_common_markers():
    """Allele frequencies in 0.1 .. 0.9: the relative error of a weight stays near 2.4e-6 (w_max / (w_min 2^22) with w = 1 / (2pq))."""
    from eagleeverything_amd import r_api
    M8, _, R = structured_panel()
    n0, n1, n2 = counts_of(M8, R)
    q, scale, used = r_api.grm_weights(n0, n1, n2)
    _, _, _, w = py_weights(n0, n1, n2)
    wa = np.array(w)[used]
    rel = np.max(np.abs(q[used] / scale - wa) / wa)
    assert used.all() and rel <= wa.max() / (wa.min() * (2.0 ** 22 - 2)) and rel < 1e-5


# ---- grm_from_gram ----
@pytest.mark.parametrize("method", ["standardized", "vanraden1"])
def test_grm_from_gram_against_the_definition(golden, method):
    from eagleeverything_amd import r_api
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    for reference in (None, np.arange(0, n, 2), np.arange(n) < 150):
        R = np.arange(n) if reference is None else (np.flatnonzero(reference) if np.asarray(reference).dtype == bool else reference)
        n0, n1, n2 = counts_of(M8, R)
        q, scale, used = r_api.grm_weights(n0, n1, n2, method=method, maf=0.2)
        assert 0 < used.sum() < L
        Q = np_wgram(M8, q)
        info = {"method": method, "scale": scale, "used": used, "n0": n0, "n1": n1, "n2": n2}
        G = r_api.grm_from_gram(Q, info, reference=reference)
        truth = direct_grm(M8, q, scale, used, method, R)
        assert G.dtype == np.float64 and G.shape == (n, n)
        assert np.max(np.abs(G - truth)) <= 1e-12 * np.max(np.abs(truth))
        assert np.max(np.abs(G - G.T)) <= 1e-13 * np.max(np.abs(G))
        assert np.max(np.abs(G[np.ix_(R, R)].sum(axis=0))) <= 1e-9 * np.max(np.abs(G))     # centred over R
    with pytest.raises(ValueError):
        r_api.grm_from_gram(Q, dict(info, used=np.zeros(L, bool)))
    with pytest.raises(ValueError):
        r_api.grm_from_gram(Q, info, reference=[0, n])
    with pytest.raises(ValueError):
        r_api.grm_from_gram(Q[:, :-1], info)


def test_grm_from_gram_in_fractions():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(8)
    M8 = rng.integers(-1, 2, size=(8, 40)).astype(np.int8)
    M8[:, 3] = 1                                                           # monomorphic over everyone
    M8[:6, 4] = -1                                                         # monomorphic over the reference only
    for reference, method in ((None, "standardized"), ([0, 1, 2, 3, 4, 5], "standardized"), ([0, 1, 2, 3, 4, 5], "vanraden1")):
        R = list(range(8)) if reference is None else reference
        n0, n1, n2 = counts_of(M8, R)
        q, scale, used = r_api.grm_weights(n0, n1, n2, method=method)
        assert not used[3] and (reference is None or not used[4])
        info = {"method": method, "scale": scale, "used": used, "n0": n0, "n1": n1, "n2": n2}
        G = r_api.grm_from_gram(np_wgram(M8, q), info, reference=reference)
        mu = [Fraction(int(M8[R, m].sum()), len(R)) for m in range(40)]
        if method == "standardized":
            den = Fraction(scale) * int(used.sum())
        else:
            den = sum(2 * ((mu[m] + 1) / 2) * (1 - (mu[m] + 1) / 2) for m in range(40) if used[m])
        for i in range(8):
            for j in range(8):
                exact = sum(int(q[m]) * (int(M8[i, m]) - mu[m]) * (int(M8[j, m]) - mu[m]) for m in range(40)) / den
                assert abs(Fraction(float(G[i, j])) - exact) <= Fraction(1, 10 ** 12) * max(abs(Fraction(float(x))) for x in G.ravel())


# ---- PCA ----
def host_grm(M8, R, method="standardized", maf=0.0):
    """The dict r_api.GRM returns, made without a device: the weights from the counts over R, Q from numpy."""
    from eagleeverything_amd import r_api
    n0, n1, n2 = counts_of(M8, R)
    q, scale, used = r_api.grm_weights(n0, n1, n2, method=method, maf=maf)
    out = {"Q": np_wgram(M8, q), "q": q, "scale": scale, "used": used, "method": method, "n0": n0, "n1": n1, "n2": n2, "reference": R}
    out["G"] = r_api.grm_from_gram(out["Q"], out, reference=R)
    return out


def assert_pca_properties(pca, labels, R, G_t, pcs_t, k):
    """What tests/test_gpu_grm.py asserts on the device's result too."""
    n = G_t.shape[0]
    assert pca["pcs"].shape == (n, k) and pca["values"].shape == (k,) and np.all(np.diff(pca["values"]) < 0)
    # the quantised weights move G by their relative error (about 2.4e-6 on this panel), no more
    assert np.max(np.abs(pca["grm"]["G"] - G_t)) <= 1e-5 * np.max(np.abs(G_t))
    U, Ut = pca["pcs"][R][:, :2], pcs_t[R][:, :2]
    assert np.max(np.abs(np.linalg.norm(pca["pcs"][R], axis=0) - 1.0)) <= 1e-12
    assert np.linalg.svd(U.T @ Ut, compute_uv=False).min() >= 1 - 1e-9     # the subspace: lambda_1 and lambda_2 are 5 % apart
    assert np.max(np.abs(pca["pcs"][300:303] - pca["pcs"][0:3])) <= 1e-10
    assert misclassified(pca["pcs"], labels, R)[0] == 0
    big = np.argmax(np.abs(pca["pcs"][R]), axis=0)
    assert np.all(pca["pcs"][R][big, np.arange(k)] > 0)                    # the sign convention
    GR = pca["grm"]["G"][np.ix_(R, R)]
    assert np.allclose(pca["explained"], pca["values"] / np.trace(GR), rtol=1e-12) and np.all(pca["explained"] > 0)


def test_pca_of_three_populations():
    from eagleeverything_amd import am, r_api
    M8, labels, R, G_t, lam_t, pcs_t = structured_truth()
    grm = host_grm(M8, R)
    pca = r_api.PCA(None, k=2, grm=grm)
    assert_pca_properties(pca, labels, R, G_t, pcs_t, 2)
    assert np.allclose(pca["values"], lam_t[:2], rtol=1e-5) and np.array_equal(pca["reference"], R) and pca["grm"] is grm
    # reference rows are the eigenvector entries themselves; every row, reference or not, is the projection
    GR = grm["G"][np.ix_(R, R)]
    assert np.max(np.abs(GR @ pca["pcs"][R] - pca["pcs"][R] * pca["values"][None, :])) <= 1e-12 * pca["values"][0]
    proj = (grm["G"][:, R] @ pca["pcs"][R]) / pca["values"][None, :]
    assert np.max(np.abs(proj - pca["pcs"])) <= 1e-13
    # an eig= callable with the other order of the values and flipped signs gives the same components
    desc = r_api.PCA(None, k=2, grm=grm, reference=R, eig=lambda A: (np.linalg.eigh(A)[0][::-1], -np.linalg.eigh(A)[1][:, ::-1]))
    assert np.array_equal(desc["values"], pca["values"]) and np.array_equal(desc["pcs"], pca["pcs"])
    # without a reference everyone centres the matrix: the three duplicates are then part of the decomposition
    allp = r_api.PCA(None, k=3, grm=host_grm(M8, np.arange(303)))
    assert allp["pcs"].shape == (303, 3) and misclassified(allp["pcs"], labels, np.arange(303))[0] == 0
    for bad in (0, 300, -1):
        with pytest.raises(ValueError):
            r_api.PCA(None, k=bad, grm=grm)
    assert r_api.PCA(None, k=299, grm=grm)["pcs"].shape == (303, 299)
    with pytest.raises(ValueError):
        r_api.PCA(None, k=2, grm=grm, reference=np.arange(299))
    X = np.ones((303, 1))
    Xp = am.add_pcs(X, pca)
    assert Xp.shape == (303, 3) and np.array_equal(Xp[:, 0], X[:, 0]) and np.array_equal(Xp[:, 1:], pca["pcs"])
    assert np.array_equal(am.add_pcs(X, pca, k=1), Xp[:, :2]) and np.array_equal(am.add_pcs(np.ones(303), pca, k=0), X)
    with pytest.raises(ValueError):
        am.add_pcs(X[:-1], pca)
    with pytest.raises(ValueError):
        am.add_pcs(X, pca, k=3)


def test_weighted_gram_rejects_bad_weights_before_the_library(tmp_path):
    from eagleeverything_amd import rcpp_api
    path = str(tmp_path / "absent.ascii")                                  # never opened: the checks come first
    for q in ([1, 2], [1, 2, 3, 4], [1, -1, 0], [0, 1 << 21, 0], [0.5, 1, 1], [float("nan"), 1, 1]):
        with pytest.raises(ValueError):
            rcpp_api.weighted_gram(path, (5, 3), q)
