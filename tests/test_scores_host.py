"""CPU: the host side of the line scores (include/eagle_hip.h section 1b''''i) -- the numpy restatement against Python integers, the
balanced base-256 digits, the quantiser and its bound, the BLUP identity of am.blup_operands and the PCA loadings identity with the
restatement standing in for the device.  No device work."""
import numpy as np
import pytest

from scores_truth import EDGES, EPS, W30, dot_bound, np_scores, py_scores


def test_line_scores_host_against_python_integers():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(1)
    G8 = rng.integers(-1, 2, (7, 13)).astype(np.int8)
    w = rng.integers(-W30, W30 + 1, (3, 13))
    w[0, :4] = (W30, -W30, W30 - 1, 0)
    truth = py_scores(G8, w)
    got = r_api.line_scores_host(G8, w)
    assert got.dtype == np.int64 and got.shape == (7, 3) and np.array_equal(got, truth)
    assert np.array_equal(np_scores(G8, w), truth)                                   # the helper the GPU tests use
    assert np.array_equal(r_api.line_scores_host(G8, w[1]), truth[:, 1:2])           # a vector is one column
    assert np.array_equal(r_api.line_scores_host(G8, w.astype(np.int32)), truth)


def test_score_digits_reconstruct_the_weights():
    from eagleeverything_amd import r_api
    w = np.concatenate([np.array(EDGES, dtype=np.int64), np.random.default_rng(2).integers(-W30, W30 + 1, 10000)])
    d = r_api.score_digits_host(w)
    assert d.dtype == np.int8 and d.shape == (4, w.size)
    assert np.array_equal(sum(d[p].astype(np.int64) << (8 * p) for p in range(4)), w)
    for x in EDGES:                                                                   # digit by digit in Python integers
        y, digs = int(x), []
        for _ in range(4):
            dp = ((y + 128) & 255) - 128
            digs.append(dp)
            y = (y - dp) >> 8
        assert y == 0 and all(-128 <= v <= 127 for v in digs)
        assert list(r_api.score_digits_host(np.array([x]))[:, 0]) == digs
    assert not r_api.score_digits_host(np.array([5, -100, 127, -128]))[1:].any()      # |w| <= 127 (and -128): one plane
    assert not r_api.score_digits_host(np.array([256, -512, 1 << 20]))[0].any()       # multiples of 256: plane 0 empty
    assert r_api.score_digits_host(np.zeros((2, 3), dtype=np.int64)).shape == (4, 2, 3)
    with pytest.raises(ValueError):
        r_api.score_digits_host(np.array([W30 + 1]))


@pytest.mark.parametrize("bits", [30, 12])
def test_quantise_weights(bits):
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(3)
    w = rng.standard_normal((500, 5)) * np.array([1.0, 1e-9, 1e7, 0.0, 3.0])[None, :]
    w[:, 4] = np.clip(w[:, 4], -3.9, 3.9)
    w[0, 4] = 4.0                                                                     # max|w| a power of two: the scale reaches 2^bits
    wq, scale = r_api.quantise_weights(w, bits=bits)
    assert wq.dtype == np.int32 and wq.shape == w.shape and scale.shape == (5,)
    m, e = np.frexp(scale)
    assert np.all(m == 0.5)                                                           # powers of two
    big = np.abs(wq).max(axis=0)
    for t in (0, 1, 2, 4):
        assert (1 << (bits - 1)) < big[t] <= (1 << bits)
        assert np.abs(w[:, t] - wq[:, t] / scale[t]).max() <= 0.5 / scale[t]          # wq / scale and the difference are exact here
        assert np.abs(w[:, t]).max() * scale[t] <= float(1 << bits) < np.abs(w[:, t]).max() * scale[t] * 2
    assert big[4] == 1 << bits
    assert scale[3] == 1.0 and not wq[:, 3].any()                                     # a zero column
    v, s = r_api.quantise_weights(w[:, 0], bits=bits)                                 # a vector: one column, a float scale
    assert isinstance(s, float) and s == scale[0] and np.array_equal(v, wq[:, 0])
    for bad in (np.nan, np.inf, -np.inf):
        w2 = w.copy()
        w2[7, 2] = bad
        with pytest.raises(ValueError):
            r_api.quantise_weights(w2, bits=bits)
    # the stated score bound: C characters in {-1, 0, +1}
    g = rng.integers(-1, 2, 500)
    for t in (0, 1, 2, 4):
        exact = float(np.dot(g, wq[:, t].astype(np.int64))) / scale[t]
        assert abs(exact - float(g @ w[:, t])) <= 0.5 * 500 / scale[t] + dot_bound(g.astype(np.float64), w[:, t])
        if bits == 30:
            assert 0.5 * 500 / scale[t] < 500 * np.abs(w[:, t]).max() * 2.0 ** -29


def test_blup_operands_identity(golden):
    from eagleeverything_amd import am
    g = golden("genoDemo_150x4998")
    M8, y, X = g["M8"], g["y"], g["X"]
    n = M8.shape[0]
    assert n == 150
    MMt = g["MMt"].astype(np.float64)
    K = MMt / MMt.max()
    K.flat[:: n + 1] += 0.95
    ve, vg = 0.7, 1.9
    op = am.blup_operands(y, X, K, ve, vg)
    assert op["beta"].shape == (X.shape[1],) and op["Py"].shape == (n,) and op["ghat"].shape == (n,)
    H = ve * np.eye(n) + vg * K
    tol = n * EPS * np.linalg.cond(H) * np.linalg.norm(y)
    assert np.abs((y - X @ op["beta"]) - (vg * (K @ op["Py"]) + ve * op["Py"])).max() <= tol
    assert np.array_equal(op["ghat"], vg * (K @ op["Py"]))
    assert np.abs(X.T @ op["Py"]).max() <= tol * np.abs(X).sum(axis=0).max()          # P X = 0


def test_pca_loadings_identity_with_the_host_restatement(golden):
    """PCA(loadings=True)'s arithmetic with line_scores_host in the place of both device calls: the projection of the panel's own
    individuals, members of the reference and the others, equals pcs within the two quantisation bounds and the fp64 sums' own."""
    from eagleeverything_amd import r_api
    from test_grm_host import counts_of, np_wgram
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    R = np.array([i for i in range(n) if i % 5 != 4])
    n0, n1, n2 = counts_of(M8, R)
    q, scale, used = r_api.grm_weights(n0, n1, n2, maf=0.01)
    grm = {"Q": np_wgram(M8, q), "q": q, "scale": scale, "used": used, "method": "standardized", "n0": n0, "n1": n1, "n2": n2, "reference": R}
    grm["G"] = r_api.grm_from_gram(grm["Q"], grm, reference=R)
    k = 4
    pca = r_api.PCA(None, k=k, grm=grm)
    assert "loadings" not in pca
    lo = r_api._pca_loadings(lambda v: r_api.line_scores_host(np.ascontiguousarray(M8.T), v), grm, R, pca["values"], pca["pcs"][R])
    assert lo["loadings"].shape == (L, k) and lo["offset"].shape == (k,) and lo["loadings_bound"].shape == (k,)
    assert not lo["loadings"][~used].any()
    wq, sc = r_api.quantise_weights(lo["loadings"])
    proj = r_api.line_scores_host(M8, wq.T).astype(np.float64) / sc[None, :] - lo["offset"][None, :]
    nu = int(used.sum())
    for a in range(k):
        # Score's bound; the loadings' bound over the used markers, in the score and in the offset; the fp64 sums of pcs and of the offset
        fp = dot_bound(grm["G"][:, R], np.abs(pca["pcs"][R][:, a])) / pca["values"][a] + dot_bound(np.ones((1, L)), np.abs(lo["loadings"][:, a]))
        bound = 0.5 * L / sc[a] + 2.0 * nu * lo["loadings_bound"][a] + 4.0 * fp
        assert np.abs(proj[:, a] - pca["pcs"][:, a]).max() <= bound, (a, np.abs(proj[:, a] - pca["pcs"][:, a]).max(), bound)
        assert bound < 1e-4 * np.abs(pca["pcs"][:, a]).max()                          # the bound says something: 4 digits below the coordinates
