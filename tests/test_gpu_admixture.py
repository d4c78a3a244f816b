"""The admixture EM step on the GPU: eagle_admixture_em (k_admix_f, k_admix_q, k_admix_ll_finish, k_admix_q_finish; include/eagle_hip.h
section 1b''''v) and r_api.Admixture on top.

Expected values: r_api.admixture_host, which tests/test_admixture_host.py holds to 40-digit arithmetic on the CPU, within the bounds of
tests/admixture_truth.py (relative 8 (max(n, L) + K + 16) 2^-53 per f' and q'; 2 n L (K + 4) 2^-53 + n L 2^-53 |l| for l).  Between
routes, between steps = 5 and five single steps and between repeated calls every comparison is ==."""
import os

import numpy as np
import pytest

import admixture_truth as truth
from test_gpu_groups import planted_panel
from test_gpu_marker_qc import ingest_text

KS = [1, 3, 16]


def same(a, b):
    return all(x.dtype == np.float64 and x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))


def check_one_step(fMt, Mt8, K, seed):
    from eagleeverything_amd import r_api, rcpp_api
    L, n = Mt8.shape
    Q, F = truth.planted_inputs(n, L, K, seed)
    Q_in, F_in = Q.copy(), F.copy()
    got = rcpp_api.admixture_em(fMt, (n, L), Q, F, 1)
    assert np.array_equal(Q, Q_in) and np.array_equal(F, F_in)        # the inputs are not modified
    assert got[2].shape == (2,)
    want = r_api.admixture_host(Mt8, Q, F, 1)
    truth.assert_close((got[0], got[1], got[2][0], got[2][1]), (want[0], want[1], want[2][0], want[2][1]), n, L, K, "device")
    # a row's K quotients v_k / s carry 2^-53 each relative to themselves (together at most 2^-53 of the sum), the sum s that divides
    # them K - 1 roundings, and the sum taken here K - 1 more: (2 K - 1) 2^-53, which is below 4 * 2^-52 up to K = 4
    assert np.max(np.abs(got[0].sum(axis=1) - 1.0)) <= (2 * K - 1) * 2.0 ** -53
    if K >= 2 and n == 1:                                              # population K - 1 has no individual: its frequencies stay
        assert np.array_equal(got[1][:, K - 1], F[:, K - 1])
    return got


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 255, 257, 1003])
def test_gpu_admixture_every_n(tmp_path, n):
    """The 16-individual tile and its ragged end, at L = 300 (19 marker tiles, the last of 12 markers)."""
    from eagleeverything_amd import rcpp_api, synth
    L = 300
    Mt8 = planted_panel(n, L, 100 + n)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    for K in KS:
        check_one_step(geno["asciifileMt"], Mt8, K, n + K)
    rcpp_api.drop_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1000])
def test_gpu_admixture_every_L(tmp_path, L):
    """The 16-marker tile, the four-wave workgroup and the marker ranges, at n = 203."""
    from eagleeverything_amd import rcpp_api, synth
    n = 203
    Mt8 = planted_panel(n, L, 200 + L)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    for K in KS:
        check_one_step(geno["asciifileMt"], Mt8, K, L + K)
    rcpp_api.drop_cache()


@pytest.mark.gpu
def test_gpu_admixture_every_K_composition_and_determinism(tmp_path):
    from eagleeverything_amd import rcpp_api, synth
    n, L = 65, 257
    Mt8 = planted_panel(n, L, 7)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    fMt = geno["asciifileMt"]
    for K in range(1, 17):
        first = check_one_step(fMt, Mt8, K, 50 + K)
        Q, F = truth.planted_inputs(n, L, K, 50 + K)
        assert same(first, rcpp_api.admixture_em(fMt, (n, L), Q, F, 1))            # a repeated call gives the same words
        if K not in (1, 5, 16):
            continue
        five = rcpp_api.admixture_em(fMt, (n, L), Q, F, 5)
        assert five[2].shape == (6,) and np.all(np.isfinite(five[2]))
        q, f, trace = Q, F, []
        for _ in range(5):
            q, f, ll = rcpp_api.admixture_em(fMt, (n, L), q, f, 1)
            trace.append(ll)
        assert same(five, (q, f, np.array([t[0] for t in trace] + [trace[-1][1]])))  # steps = 5 is five calls of steps = 1
        assert all(trace[i][1] == trace[i + 1][0] for i in range(4))                 # l after a step is l before the next
        zero = rcpp_api.admixture_em(fMt, (n, L), Q, F, 0)
        assert same(zero, (Q, F, five[2][:1]))                                       # steps = 0: Q and F untouched and one l
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 2. routes
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["genoDemo_150x4998", "synth_203x1531"])
def test_gpu_admixture_resident_sidecar_windows_text(golden, tmp_path, monkeypatch, case):
    from eagleeverything_amd import r_api, rcpp_api
    M8 = golden(case)["M8"]
    n, L = M8.shape
    K, steps = 5, 3
    Q, F = truth.planted_inputs(n, L, K, 11)
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    fMt = geno["asciifileMt"]
    mmt = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L))
    whole = rcpp_api.marker_counts(fMt, (n, L))
    res = rcpp_api.admixture_em(fMt, (n, L), Q, F, steps)                            # the image the converter left resident
    host = r_api.admixture_host(np.ascontiguousarray(M8.T), Q, F, 1)
    one = rcpp_api.admixture_em(fMt, (n, L), Q, F, 1)
    truth.assert_close((one[0], one[1], one[2][0], one[2][1]), (host[0], host[1], host[2][0], host[2][1]), n, L, K, case)
    assert res[2].shape == (steps + 1,) and res[2][0] == one[2][0] and res[2][1] == one[2][1] and res[2][-1] > res[2][0]
    # the cached images were read, not written: the passes before give the bits they gave
    assert np.array_equal(rcpp_api.marker_counts(fMt, (n, L)), whole)
    assert np.array_equal(rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L)), mmt)
    rcpp_api.drop_cache()                                                            # from the sidecar, made resident
    assert os.path.exists(fMt + ".e2b")
    assert same(rcpp_api.admixture_em(fMt, (n, L), Q, F, steps), res)
    rcpp_api.drop_cache()                                                            # in row windows of 256 markers (test_gpu_groups.py's setting)
    n_pad = (n + 255) // 256 * 256
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr((256 * n_pad - 16) / 1e9))
    assert same(rcpp_api.admixture_em(fMt, (n, L), Q, F, steps), res)
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")                                     # the same windows from the text
    assert same(rcpp_api.admixture_em(fMt, (n, L), Q, F, steps), res)
    rcpp_api.drop_cache()


@pytest.mark.gpu
def test_gpu_admixture_window_that_ends_inside_a_range(tmp_path, monkeypatch):
    """1003 individuals are 63 tiles, so the plan cuts 1531 markers into 32 ranges of 48: windows of 256 rows end inside every third
    range, whose accumulator then passes through the partials buffer."""
    from eagleeverything_amd import rcpp_api, synth
    n, L, K = 1003, 1531, 4
    Mt8 = planted_panel(n, L, 9)
    Q, F = truth.planted_inputs(n, L, K, 12)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    res = rcpp_api.admixture_em(geno["asciifileMt"], (n, L), Q, F, 2)
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr((256 * 1024 - 16) / 1e9))
    assert same(rcpp_api.admixture_em(geno["asciifileMt"], (n, L), Q, F, 2), res)
    rcpp_api.drop_cache()


@pytest.mark.gpu
def test_gpu_admixture_on_view_alias(golden, tmp_path, monkeypatch):
    from eagleeverything_amd import r_api, rcpp_api, synth
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    K, steps = 5, 3
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    na = np.array([1, 2, 57, 130, 203])                                              # 1-based, as R hands them over
    kept = np.setdiff1d(np.arange(n), na - 1)
    Q, F = truth.planted_inputs(n - 5, L, K, 13)                                     # one row per KEPT individual
    (tmp_path / "kept").mkdir()
    plain = synth.write_geno_pair(str(tmp_path / "kept"), np.ascontiguousarray(M8[kept].T))
    res = rcpp_api.admixture_em(plain["asciifileMt"], (n - 5, L), Q, F, steps)       # the kept individuals as a panel of their own
    dims = r_api.ReshapeM(geno["asciifileM"], geno["asciifileMt"], na, (n, L), view=True)
    assert dims[0] == n - 5
    assert same(rcpp_api.admixture_em(geno["asciifileMt"] + "tmp", (n - 5, L), Q, F, steps), res)
    rcpp_api.drop_cache()                                                            # the same alias from the source's sidecar, in windows
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr(2 * 256 * 256 / 1e9))
    assert same(rcpp_api.admixture_em(geno["asciifileMt"] + "tmp", (n - 5, L), Q, F, steps), res)
    with pytest.raises(ValueError):
        rcpp_api.admixture_em(geno["asciifileMt"] + "tmp", (n - 5, L), truth.planted_inputs(n, L, K, 13)[0], F, steps)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 3. end to end
@pytest.mark.gpu
def test_gpu_admixture_end_to_end(tmp_path):
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    n, L, K = 120, 600, 3
    Mt8, Qt, _ = truth.planted_panel(n, L, K, 1)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    r = r_api.Admixture(geno, K, seed=1)
    tr = r["loglik"]
    corr = truth.best_permutation_corr(r["Q"], Qt)
    print("iterations %d, converged %s, l %.10g, mean column correlation %.4f" % (r["iterations"], r["converged"], tr[-1], corr))
    assert r["converged"] and np.all(np.diff(tr) >= 0.0)                             # the trace never falls
    assert corr >= 0.98
    assert r["Q"].shape == (n, K) and r["F"].shape == (K, L) and np.all(np.diff(r["Q"].mean(axis=0)) <= 0.0)
    fst = r_api.Fst(geno, r["assignment"])                                           # argmax groups feed what takes groups=
    assert np.isfinite(fst["genome"][0]) and fst["genome"][0] > 0.0
    assert am.add_ancestry(np.ones(n), r).shape == (n, K)
    rcpp_api.drop_cache()
