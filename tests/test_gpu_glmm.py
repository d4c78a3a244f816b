"""The logistic mixed model on the GPU: eagle_glmm_spa (k_glmm_spa, csrc/eagle_glmm.hip) and glmm.GLMM on top.

Expected values: the 40-digit roots of tests/glmm_truth.py with the allowance its docstring derives (the one tests/test_glmm_host.py
holds the numpy restatement to), the restatement for the codes, and for GLMM the all-host analysis.  Device against device (routes, a
second call, poisoned allocations) is ==.  Every call uses tol = 1e-10."""
import os
import subprocess
import sys

import numpy as np
import pytest

import glmm_truth as truth
from conftest import ROOT
from test_glmm_host import check_against_truth
from test_gpu_marker_qc import ingest_text

TOL = 1e-10


def device_panel(tmp_path, n, L, c, rows=None):
    """spa on the panel glmm_truth.panel(n, L, c) at cutoff 0 and 2 against the truth (every marker, or `rows` of them) and against the
    restatement's codes (every marker)."""
    from eagleeverything_amd import glmm, rcpp_api, synth
    Mt8, mu, r, X, vs = truth.panel(n, L, c, 100 + n)
    V = glmm.spa_host(Mt8, mu, r, X, cutoff=1e9)[0][:, 1] * vs                  # an operand: V*, scaled where the fixture says so
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    out = {}
    for cutoff in (0.0, 2.0):
        stat, info = glmm.spa(geno["asciifileMt"], (n, L), mu, r, X, vara=V, cutoff=cutoff, tol=TOL)
        assert stat.shape == (L, 7) and info.shape == (L, 2) and stat.dtype == np.float64 and info.dtype == np.int32
        check_against_truth("device n%d L%d c%d cutoff %g" % (n, L, c, cutoff), Mt8, mu, r, X, V, stat, info, cutoff, rows)
        hstat, hinfo = glmm.spa_host(Mt8, mu, r, X, vara=V, cutoff=cutoff, tol=TOL)
        assert np.array_equal(info[:, 0], hinfo[:, 0]), (n, L, c, cutoff)
        assert np.array_equal(np.isnan(stat), np.isnan(hstat))
        out[cutoff] = (stat, info)
    # without vara V = V*: z^2 V* = T^2
    s0, i0 = glmm.spa(geno["asciifileMt"], (n, L), mu, r, X, cutoff=0.0, tol=TOL)
    ok = i0[:, 0] != 2
    assert np.all(np.abs(s0[ok, 2] ** 2 * s0[ok, 1] - s0[ok, 0] ** 2) <= 1e-12 * s0[ok, 0] ** 2)
    rcpp_api.drop_cache()
    return out


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 63, 64, 65, 257])
def test_gpu_spa_every_n(tmp_path, n):
    """The 64-lane chunk edge and n no multiple of the MFMA step's four individuals, at L = 5; mu around 0.05, rare alleles and the
    planted markers: monomorphic (2), carriers = cases beyond the support (3), a common marker (4 at cutoff 2), and with c = 4 the
    opposite tail without mass (+ 256) at n = 64 and 65."""
    out = device_panel(tmp_path, n, 5, 1 if n == 5 else 4)
    code = out[2.0][1][:, 0]
    assert code[4] == 2 and code[1] == 3
    if n in (64, 65):
        assert code[3] == 256


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 5, 130])
def test_gpu_spa_every_L(tmp_path, L):
    """A single marker, L no multiple of the four waves of a workgroup, 33 workgroups; at n = 65.  At L = 130 the truth is taken for
    the first twelve markers and the planted ones, the codes of all from the restatement."""
    rows = None if L <= 5 else list(range(12)) + list(range(L - 4, L))
    device_panel(tmp_path, 65, L, 4, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [1, 4, 15])
def test_gpu_spa_every_c(tmp_path, c):
    """Fifteen zero columns of the padded image, twelve, and one; an odd c reads a zero column in its last pair."""
    device_panel(tmp_path, 65, 5, c)


@pytest.mark.gpu
def test_gpu_spa_max_iter(tmp_path):
    from eagleeverything_amd import glmm, rcpp_api, synth
    Mt8, mu, r, X, vs = truth.panel(65, 5, 4, 165)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    stat, info = glmm.spa(geno["asciifileMt"], (65, 5), mu, r, X, cutoff=0.0, tol=TOL, max_iter=1)
    hstat, hinfo = glmm.spa_host(Mt8, mu, r, X, cutoff=0.0, tol=TOL, max_iter=1)
    assert np.array_equal(info, hinfo) and (info[:, 0] == 1).sum() >= 2 and np.all(info[info[:, 0] == 1, 1] == 1)
    assert np.all(np.isnan(stat[info[:, 0] == 1][:, 3:]))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 2. routes
def route_operands(n):
    _, mu, r, X, _ = truth.panel(n, 5, 4, 300 + n)
    return mu, r, X


@pytest.mark.gpu
def test_gpu_spa_routes_are_bit_equal(golden, tmp_path, monkeypatch):
    """n = 203, L = 300: the resident image, a second call on the same context, the sidecar made resident, two row windows of 256 with a
    short last one, the same windows from the text without a sidecar: the same bits, because a wave's result depends on its marker's
    row and the per-call operands alone."""
    from eagleeverything_amd import glmm, rcpp_api
    M8 = np.ascontiguousarray(golden("synth_203x1531")["M8"][:, :300])
    n, L = M8.shape
    mu, r, X = route_operands(n)
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    fMt = geno["asciifileMt"]
    stat, info = glmm.spa(fMt, (n, L), mu, r, X, cutoff=0.0, tol=TOL)           # the image the converter left resident
    assert (info[:, 0] & 255 == 0).mean() > 0.9 and info[:, 1].max() > 4
    s1, i1 = glmm.spa(fMt, (n, L), mu, r, X, cutoff=0.0, tol=TOL)               # a second call on the same context
    assert np.array_equal(s1, stat, equal_nan=True) and np.array_equal(i1, info)
    rcpp_api.drop_cache()                                                       # from the sidecar, made resident
    s2, i2 = glmm.spa(fMt, (n, L), mu, r, X, cutoff=0.0, tol=TOL)
    assert np.array_equal(s2, stat, equal_nan=True) and np.array_equal(i2, info)
    rcpp_api.drop_cache()                                                       # in row windows of 256 markers
    n_pad = (n + 255) // 256 * 256
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr((256 * n_pad - 16) / 1e9))
    s3, i3 = glmm.spa(fMt, (n, L), mu, r, X, cutoff=0.0, tol=TOL)
    assert np.array_equal(s3, stat, equal_nan=True) and np.array_equal(i3, info)
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")                                # the same windows from the text
    s4, i4 = glmm.spa(fMt, (n, L), mu, r, X, cutoff=0.0, tol=TOL)
    assert np.array_equal(s4, stat, equal_nan=True) and np.array_equal(i4, info)
    # vara rides with its window
    V = stat[:, 1] * np.linspace(0.7, 1.3, L)
    s5, i5 = glmm.spa(fMt, (n, L), mu, r, X, vara=V, cutoff=0.0, tol=TOL)
    monkeypatch.delenv("EAGLE_HIP_MAX_RESIDENT_GB")
    monkeypatch.delenv("EAGLE_HIP_SIDECAR")
    rcpp_api.drop_cache()
    s6, i6 = glmm.spa(fMt, (n, L), mu, r, X, vara=V, cutoff=0.0, tol=TOL)
    assert np.array_equal(s5, s6, equal_nan=True) and np.array_equal(i5, i6)
    ok = i6[:, 0] != 2
    assert np.all(np.abs(s6[ok, 2] * np.sqrt(V[ok]) - s6[ok, 0]) <= 1e-13 * np.abs(s6[ok, 0]))
    rcpp_api.drop_cache()


@pytest.mark.gpu
def test_gpu_spa_on_view_alias(golden, tmp_path, monkeypatch):
    from eagleeverything_amd import am, glmm, rcpp_api
    M8 = np.ascontiguousarray(golden("synth_203x1531")["M8"][:, :300])
    n, L = M8.shape
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    na = np.array([1, 2, 57, 130, 203])                                         # 1-based, as R hands them over
    kept = np.setdiff1d(np.arange(n), na - 1)
    sub = ingest_text(tmp_path, "k", np.ascontiguousarray(M8[kept]))             # the kept individuals as a panel of their own
    mu, r, X = route_operands(n - 5)                                            # one entry per KEPT individual
    want = glmm.spa(sub["asciifileMt"], (n - 5, L), mu, r, X, cutoff=0.0, tol=TOL)
    view = am.reshape_geno(geno, na, view=True)
    assert list(view["dim_of_ascii_M"]) == [n - 5, L]
    got = glmm.spa(view["asciifileMt"], (n - 5, L), mu, r, X, cutoff=0.0, tol=TOL)
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])
    rcpp_api.drop_cache()                                                       # the same alias from the source's sidecar, in windows
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr(2 * 256 * 256 / 1e9))
    got = glmm.spa(view["asciifileMt"], (n - 5, L), mu, r, X, cutoff=0.0, tol=TOL)
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 3. the interface
@pytest.mark.gpu
def test_gpu_GLMM_end_to_end(tmp_path):
    """120 x 600 with sib-like pairs, a covariate, a causal marker, rare planted markers and two individuals without a status, against the
    all-host analysis (K, null_fit, V = m'Pm and spa_host in numpy): T within 1e-12 relative, V within the scan's gate of 1e-7, the
    codes equal, and ln p within what V's gate implies -- |d ln p / d ln V| 1e-7, the derivative from the restatement at V (1 +- 1e-4) --
    plus the allowance of glmm_truth for each of the two (the planted and the first SPA markers; the truth is taken for twelve)."""
    from eagleeverything_amd import glmm, r_api, rcpp_api, synth
    n0, L, causal = 120, 600, 77
    Mt8 = synth.genotypes_marker_major(n0, L, seed=71)
    rng = np.random.default_rng(81)
    for i in range(0, n0 - 1, 2):                                               # sib-like pairs
        mix = rng.random(L) < 0.8
        Mt8[mix, i + 1] = Mt8[mix, i]
    x = rng.standard_normal(n0)
    Mt8[causal] = np.repeat(rng.binomial(2, 0.4, n0 // 2), 2) - 1
    eta = -1.8 + 1.6 * (Mt8[causal] + 1.0) + 0.4 * x + 2.0 * np.repeat(rng.standard_normal(n0 // 2), 2)
    st = (rng.random(n0) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    cases = np.flatnonzero(st == 1)
    for k, m in enumerate((5, 6, 7)):                                           # rare alleles whose carriers are mostly cases
        Mt8[m] = -1
        Mt8[m, cases[4 * k:4 * k + 4 + k]] = 0
        if k:
            Mt8[m, np.flatnonzero(st == 0)[k]] = 0
    Mt8[8] = -1                                                                 # monomorphic
    st[[10, 50]] = np.nan
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    names = ["snp%d" % j for j in range(L)]
    Xall = np.column_stack([np.ones(n0), x])
    out = r_api.GLMM(geno, st, Xall, tol=TOL, map=names)
    keep = np.isfinite(st)
    n = int(keep.sum())
    assert out["n_used"] == n == 118 and list(out["indxNA"]) == [51, 11] and out["names"] == names
    # ---- the all-host analysis
    y, X = st[keep], Xall[keep]
    M = Mt8[:, keep].T.astype(np.float64)
    K = M @ M.T
    K = K / K.max() + 0.95 * np.eye(n)
    fit = glmm.null_fit(y, X, K)
    assert fit["converged"] and out["null"]["converged"] and out["null"]["iterations"] == fit["iterations"]
    assert abs(out["null"]["tau"] - fit["tau"]) <= 1e-9 * max(fit["tau"], 1.0) and np.allclose(out["null"]["alpha"], fit["alpha"], rtol=0, atol=1e-9)
    V = np.einsum("li,ij,lj->l", M.T, fit["P"], M.T)
    hstat, hinfo = glmm.spa_host(Mt8[:, keep], fit["mu"], y - fit["mu"], X, fit["A"], V, tol=TOL)
    host = glmm.glmm_columns(hstat, hinfo, V)
    ok = hinfo[:, 0] != 2
    Vdev = 1.0 / out["se"] ** 2
    Tdev = out["beta"] * Vdev
    print("worst T error %.3g relative, worst V error %.3g" % (np.max(np.abs(Tdev[ok] / hstat[ok, 0] - 1.0)), np.max(np.abs(Vdev[ok] / V[ok] - 1.0))))
    assert np.all(np.abs(Tdev[ok] - hstat[ok, 0]) <= 1e-12 * np.abs(hstat[ok, 0]))
    assert np.all(np.abs(Vdev[ok] / V[ok] - 1.0) <= 1e-7)
    assert np.array_equal(out["code"], hinfo[:, 0]) and out["code"][8] == 2 and np.isnan(out["p"][8])
    assert np.array_equal(out["spa_used"], hinfo[:, 0] & 255 == 0) and 5 <= out["spa_used"].sum() <= L // 4
    assert np.all(out["spa_used"][[5, 7]]) and np.all(out["code"][~out["spa_used"] & ok] == 4) and fit["tau"] > 0.1
    # the fixture keeps every |T| above 1e-4 of its terms' magnitudes, or 1e-12 of T would be below the last bit of the sum
    assert np.min(np.abs(hstat[ok, 0]) / np.abs((Mt8[:, keep][ok] + 1.0) * (y - fit["mu"])).sum(axis=1)) > 1e-4
    assert np.allclose(out["score"][ok], host["score"][ok], rtol=3e-7) and np.allclose(out["p_norm"][ok], host["p_norm"][ok], rtol=1e-5)
    spa_rows = [5, 7] + [int(m) for m in np.flatnonzero(out["spa_used"]) if m not in (5, 7)][:10]
    for m in spa_rows:
        t = truth.truth(fit["mu"], X, Mt8[m, keep] + 1.0, y - fit["mu"], V=V[m], A=fit["A"])
        lnp = {}
        for f in (1.0 - 1e-4, 1.0 + 1e-4):
            s, i = glmm.spa_host(Mt8[m:m + 1, keep], fit["mu"], y - fit["mu"], X, fit["A"], [V[m] * f], cutoff=0.0, tol=TOL)
            lnp[f] = truth.lnp_of(s[0])
        dlnp = abs(lnp[1.0 + 1e-4] - lnp[1.0 - 1e-4]) / 2e-4
        allow = dlnp * 1e-7 + 2.0 * truth.allowance(t, TOL)
        err = abs(np.log(out["p_spa"][m]) - np.log(host["p_spa"][m]))
        print("marker %d: ln p %.3f, device - host %.3g, allowed %.3g" % (m, np.log(host["p_spa"][m]), err, allow))
        assert err <= allow, (m, err, allow)
    assert np.array_equal(out["p"][out["spa_used"]], out["p_spa"][out["spa_used"]])
    assert np.array_equal(out["p"][~out["spa_used"]], out["p_norm"][~out["spa_used"]], equal_nan=True)
    p = out["p"].copy()
    p[[5, 6, 7]] = np.nan
    assert int(np.nanargmin(p)) == causal and out["beta"][causal] > 0
    from scipy.special import chdtri
    assert abs(out["lambda_gc"] - np.nanmedian(out["score"]) / chdtri(1.0, 0.5)) <= 1e-12
    # tau = 0.0: the model of Logistic, whose score test this is
    o0 = r_api.GLMM(geno, st, Xall, tau=0.0, tol=TOL)
    lg = r_api.Logistic(geno, st, Xall, firth="ml", tol=TOL)
    assert o0["null"]["tau"] == 0.0 and np.allclose(o0["score"][ok], lg["score"][ok], rtol=1e-5, atol=1e-8)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 4. poisoned allocations
CHILD = r"""
import os, sys
import numpy as np
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import glmm_truth as truth
from eagleeverything_amd import glmm, rcpp_api, synth
out, work = sys.argv[2], sys.argv[3]
res = []
for tag, n, L in (("big", 406, 600), ("small", 203, 300)):                      # the call under test runs behind one about twice as large
    Mt8 = synth.genotypes_marker_major(n, L, seed=81)
    _, mu, r, X, _ = truth.panel(n, 5, 4, 300 + n)
    d = os.path.join(work, tag)
    os.makedirs(d)
    geno = synth.write_geno_pair(d, Mt8)
    V = np.linspace(0.5, 1.5, L) * 0.04 * n
    for vara in (None, V):
        res.append(glmm.spa(geno["asciifileMt"], (n, L), mu, r, X, vara=vara, cutoff=0.0, tol=1e-10))
small = res[2:]
np.savez(out, s0=small[0][0], i0=small[0][1], s1=small[1][0], i1=small[1][1])
rcpp_api.close_all()
print("child ok")
"""


@pytest.mark.gpu
def test_gpu_spa_on_poisoned_allocations(tmp_path):
    """Every device allocation of eagle_glmm_spa goes through DevBuf, so EAGLE_HIP_POISON fills the staged images, vara, stat and info
    with a byte before the call writes them: the call at n = 203, L = 300, behind the same call on a panel twice as large, gives under
    0xFF, 0x7F and 0x55 the bytes it gives on clean memory.  Each run is a fresh process."""
    results = {}
    for fill in (None, 0xFF, 0x7F, 0x55):
        env = dict(os.environ)
        env.pop("EAGLE_HIP_POISON", None)
        if fill is not None:
            env["EAGLE_HIP_POISON"] = str(fill)
        work = tmp_path / ("w%s" % fill)
        work.mkdir()
        out = str(tmp_path / ("out%s.npz" % fill))
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD, ROOT, out, str(work)], env=env, capture_output=True, text=True)
        assert r.returncode == 0 and "child ok" in r.stdout, (fill, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        with np.load(out) as z:
            results[fill] = {k: z[k].tobytes() for k in z.files}
    clean = results[None]
    assert len(clean["s0"]) == 300 * 7 * 8 and len(clean["i0"]) == 300 * 2 * 4
    codes = np.frombuffer(clean["i0"], dtype=np.int32).reshape(300, 2)[:, 0]
    assert (codes & 255 == 0).mean() > 0.9
    for fill in (0xFF, 0x7F, 0x55):
        assert results[fill] == clean, "fill 0x%02X changes the result" % fill
