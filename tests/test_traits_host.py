"""AM_traits and the eigenbasis variance components (eagleeverything_amd/am.py) on the host.

emma_REMLE_eig / emma_MLE_eig must reproduce emma_REMLE / emma_MLE from lam, U = eigh(K) alone.  AM_traits runs with a numpy
stand-in for the spectral calls (Z = Mt U in fp64 on the host) and must pick, trait by trait, what AM() picks with the oracle
backend on the same trait with the union of the NA rows."""
import numpy as np
import pytest

from eagleeverything_amd import am, rcpp_api, r_api, synth

from test_am_driver import OracleBackend


def _demo_K(golden):
    g = golden("genoDemo_150x4998")
    K = g["MMt"] / g["MMt_norm_max"] + 0.95 * np.eye(g["MMt"].shape[0])
    return g, K


def _assert_same(ref, got, keys):
    for k in keys:
        assert got[k] == pytest.approx(ref[k], rel=1e-9, abs=0.0), k


@pytest.mark.parametrize("q", [3, 5, 12])
def test_emma_eig_matches_emma_on_demo_K(golden, q):
    g, K = _demo_K(golden)
    M = g["M8"].astype(np.float64)
    X = g["X"] if q == 3 else np.column_stack([g["X"], M[:, 7 + 311 * np.arange(q - 3)]])
    lam, U = np.linalg.eigh(K)
    y = g["y"]
    _assert_same(am.emma_REMLE(y, X, K), am.emma_REMLE_eig(lam, U.T @ X, U.T @ y), ("REML", "delta", "ve", "vg"))
    _assert_same(am.emma_MLE(y, X, K), am.emma_MLE_eig(lam, U.T @ X, U.T @ y), ("ML", "delta", "ve", "vg"))
    _assert_same(am.emma_MLE(y, X, K, llim=-100, ulim=100), am.emma_MLE_eig(lam, U.T @ X, U.T @ y, llim=-100, ulim=100),
                 ("ML", "delta", "ve", "vg"))


@pytest.mark.parametrize("seed", [1, 2])
def test_emma_eig_matches_emma_on_random_spd(seed):
    rng = np.random.default_rng(seed)
    n = 120
    A = rng.standard_normal((n, 300))
    K = A @ A.T / 300 + 0.1 * np.eye(n)
    lam, U = np.linalg.eigh(K)
    X = np.column_stack([np.ones(n), rng.standard_normal((n, 3))])
    y = X @ rng.standard_normal(4) + A[:, :5].sum(axis=1) / 3 + rng.standard_normal(n)
    _assert_same(am.emma_REMLE(y, X, K), am.emma_REMLE_eig(lam, U.T @ X, U.T @ y), ("REML", "delta", "ve", "vg"))
    _assert_same(am.emma_MLE(y, X, K), am.emma_MLE_eig(lam, U.T @ X, U.T @ y), ("ML", "delta", "ve", "vg"))


def test_emma_eig_duplicated_column_follows_emma(golden):
    g, K = _demo_K(golden)
    lam, U = np.linalg.eigh(K)
    X = np.column_stack([g["X"], g["X"][:, 1]])
    assert am.emma_REMLE_eig(lam, U.T @ X, U.T @ g["y"]) == am.emma_REMLE(g["y"], X, K)
    assert am.emma_MLE_eig(lam, U.T @ X, U.T @ g["y"]) == am.emma_MLE(g["y"], X, K)


def test_traits_passes_group_whole_traits():
    assert rcpp_api.spectral_traits_passes([5]) == 1
    assert rcpp_api.spectral_traits_passes([5] * 16) == 1            # 96 lin + 16 quad columns: 7 tiles
    assert rcpp_api.spectral_traits_passes([5] * 17) == 2            # 102 lin columns (7 tiles) + 17 quad columns (2 tiles)
    assert rcpp_api.spectral_traits_passes([5] * 64) == 4
    assert rcpp_api.spectral_traits_passes([31] * 3) == 1            # 96 lin columns (6 tiles) + 1 quad tile
    assert rcpp_api.spectral_traits_passes([31] * 4) == 2            # 128 lin columns + 1 quad tile would be 9
    for bad in ([], [0], [32]):
        with pytest.raises(ValueError):
            rcpp_api.spectral_traits_passes(bad)


class _HostSpectral:
    """numpy stand-in for spectral_prepare / spectral_scan_traits / spectral_rows: Z = Mt U in fp64, the formulas of
    include/eagle_hip.h section 1d, the in-model rule and find_qtl.R's arg-max."""

    def __init__(self):
        self.Z = None
        self.calls = 0

    def prepare(self, f_name_ascii, dims, U, max_memory_in_Gbytes=8.0, device=0):
        L, n = int(dims[0]), int(dims[1])
        raw = np.frombuffer(open(f_name_ascii, "rb").read(), dtype=np.uint8).reshape(L, n + 1)[:, :n]
        self.Z = (raw.astype(np.float64) - ord("1")) @ U

    def scan(self, lam, UtX_list, UtY, varE, varG, n_markers, full=False, device=0):
        self.calls += 1
        UtY = np.asarray(UtY).reshape(lam.size, -1)
        idx, mx, A, V = [], [], [], []
        for t, Ut in enumerate(UtX_list):
            d = 1.0 / (varE[t] + varG[t] * lam)
            C = np.linalg.inv(Ut.T @ (d[:, None] * Ut))
            c1 = C @ (Ut.T @ (d * UtY[:, t]))
            Q = self.Z @ (d[:, None] * Ut)
            quad = (self.Z * self.Z) @ d
            r = quad - np.einsum("ij,jk,ik->i", Q, C, Q)
            inm = ~(r > 1e-12 * quad)
            a = np.where(inm, 0.0, varG[t] * (self.Z @ (d * UtY[:, t]) - Q @ c1))
            v = np.where(inm, 0.0, varG[t] ** 2 * r)
            with np.errstate(all="ignore"):
                tsq = a * a / v
            i = int(np.flatnonzero(tsq == np.nanmax(tsq))[0])
            idx.append(i + 1)
            mx.append(tsq[i])
            A.append(a)
            V.append(v)
        res = {"index": np.array(idx), "tsqmax": np.array(mx)}
        if full:
            res["a"], res["vara"] = np.column_stack(A), np.column_stack(V)
        return res

    def rows(self, idx, device=0):
        return self.Z[np.atleast_1d(idx)].T.copy()


def _four_traits(g):
    Mt8 = np.ascontiguousarray(g["M8"].T)
    traits = [g["y"]]
    for nqtl, beta, seed in ((2, 1.0, 3), (3, 0.8, 5), (4, 0.7, 9)):
        traits.append(synth.trait(Mt8, nqtl=nqtl, beta=beta, seed=seed)[0])
    Y = np.column_stack(traits)
    Y[[4, 40, 77, 120], 2] = np.nan
    return Mt8, Y


def test_am_traits_picks_what_am_picks_cpu(oracle, golden, tmp_path, monkeypatch):
    g = golden("genoDemo_150x4998")
    Mt8, Y = _four_traits(g)
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    ob = OracleBackend(oracle)
    fake = _HostSpectral()
    monkeypatch.setattr(r_api, "calcMMt", lambda geno, availmemGb, ncpu, sel, quiet, device=0: ob.calcMMt(geno, availmemGb, ncpu, sel, quiet))
    monkeypatch.setattr(rcpp_api, "spectral_prepare", fake.prepare)
    monkeypatch.setattr(rcpp_api, "spectral_scan_traits", fake.scan)
    monkeypatch.setattr(rcpp_api, "spectral_rows", fake.rows)
    file_reshape = am.reshape_geno
    monkeypatch.setattr(am, "reshape_geno", lambda geno, indxNA, view=False, device=0: file_reshape(geno, indxNA))
    maxit = 6
    res = am.AM_traits(Y, g["X"], geno, maxit=maxit)
    assert len(res) == Y.shape[1]
    union = np.isnan(Y).any(axis=1)
    assert fake.calls <= maxit                                        # one batched call per round
    for t in range(Y.shape[1]):
        y = Y[:, t].copy()
        y[union] = np.nan
        ref = am.AM(y, g["X"], geno, maxit=maxit, backend=ob)
        assert res[t]["all_picks"] == ref["all_picks"] and res[t]["selected_loci"] == ref["selected_loci"], t
        np.testing.assert_allclose(res[t]["extBIC_trace"], ref["extBIC_trace"], rtol=1e-8)
        np.testing.assert_allclose(res[t]["extBIC"], ref["extBIC"], rtol=1e-8)
        np.testing.assert_allclose([res[t]["ve"], res[t]["vg"]], [ref["ve"], ref["vg"]], rtol=1e-6)
        np.testing.assert_array_equal(res[t]["indxNA"], ref["indxNA"])
        assert res[t]["dim_of_ascii_M"] == ref["dim_of_ascii_M"]
        assert len(ref["all_picks"]) >= 1


def test_am_traits_rejects_too_many_columns_before_gpu_work(golden):
    g = golden("genoDemo_150x4998")
    geno = {"asciifileM": "/nonexistent/M", "asciifileMt": "/nonexistent/Mt", "dim_of_ascii_M": (150, 4998)}
    with pytest.raises(ValueError, match="31"):
        am.AM_traits(np.column_stack([g["y"], g["y"]]), g["X"], geno, maxit=30)
