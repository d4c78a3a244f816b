"""max(T) permutation testing on the GPU: eagle_maxt (k_maxt_keys, the bitonic sort kernels, k_maxt_operand, k_maxt_sv, k_maxt_tile<P, RB>,
k_maxt_finish) and the r_api interface on top.

Expected values: r_api.maxt_host, which tests/test_maxt_host.py holds to plain loops on Python ints on the CPU.  Every sum is an integer and
the key is two correctly rounded fp64 operations on exact operands: every comparison is == on all six outputs."""
import numpy as np
import pytest

from test_gpu_marker_qc import ingest_text

KEYS = ("d_obs", "V", "key_obs", "count1", "maxkey", "argmax")
EDGES = {1: 127, 2: 16383, 3: 1000000}                                     # the largest trait value of a P-plane operand


def planted_panel(n, L, seed):
    """Random genotypes with a monomorphic marker (L - 1) and a duplicate of marker 0 (L - 2) where there is room."""
    from eagleeverything_amd import synth
    Mt8 = synth.genotypes_marker_major(n, L, seed=seed)
    if L >= 4:
        Mt8[L - 1] = -1
        Mt8[L - 2] = Mt8[0]
    return Mt8


def planted_trait(n, P, seed):
    """Values in [-tmax, tmax] of a P-plane operand with the digit edges at both ends of every 128-individual chunk: +tmax at the first
    individual of a chunk, -tmax at its last, and one step inside the next-lower plane count next to them."""
    rng = np.random.default_rng(seed)
    tmax = EDGES[P]
    low = {1: 1, 2: 128, 3: 16384}[P]
    t = rng.integers(-tmax, tmax + 1, n)
    for b in range(0, n, 128):
        t[b] = tmax
        if b + 1 < n:
            t[b + 1] = -low
        e = min(b + 127, n - 1)
        if e > b + 1:
            t[e] = -tmax
            t[e - 1] = low
    if n == 3:
        t[:] = (tmax, -low, -tmax)
    return t.astype(np.int64)


def same(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        a, b = (got[k].view(np.uint64), want[k].view(np.uint64)) if got[k].dtype == np.float64 else (got[k], want[k])
        assert np.array_equal(a, b), (what, k)


def check(fMt, Mt8, t, used=None, strata=None, seed=0, first=1, R=5, perm=None, **kw):
    from eagleeverything_amd import r_api, rcpp_api
    L, n = Mt8.shape
    want = r_api.maxt_host(Mt8, t, used, strata, seed, first, R, perm=perm)
    got = rcpp_api.maxt(fMt, (n, L), t, used=used, strata=strata, seed=seed, first=first, R=R, perm=perm, **kw)
    same(got, want, (n, L, R, first))
    return got


def write_pair(tmp_path, Mt8):
    from eagleeverything_amd import rcpp_api, synth
    rcpp_api.drop_cache()
    return synth.write_geno_pair(str(tmp_path), Mt8)["asciifileMt"]


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 15, 16, 17, 127, 128, 129, 257, 1003])
def test_gpu_maxt_every_n(tmp_path, n):
    """The 16-byte piece, the MFMA k-step of 32 and the 128-byte chunk at L = 200 (two tiles, the last of 72 markers), for one, two and
    three digit planes with the digit edges at both ends of every chunk; a monomorphic and a duplicated marker ride along."""
    from eagleeverything_amd import rcpp_api
    L = 200
    Mt8 = planted_panel(n, L, 100 + n)
    fMt = write_pair(tmp_path, Mt8)
    for P in (1, 2, 3):
        got = check(fMt, Mt8, planted_trait(n, P, n + P), seed=n, R=33)
        assert got["V"][L - 1] == 0 and got["key_obs"][L - 1] == 0.0 and got["count1"][L - 1] == 33
        assert got["count1"][L - 2] == got["count1"][0] and got["d_obs"][L - 2] == got["d_obs"][0] and not np.any(got["argmax"] == L - 2)
    check(fMt, Mt8, np.arange(n) % 2, seed=1, R=33)                        # a 0/1 case indicator: one plane
    rcpp_api.drop_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 127, 128, 129, 257])
def test_gpu_maxt_every_L(tmp_path, L):
    """The 128-marker tile at n = 203: one marker, one short of a tile, a tile, one more, two tiles and one marker."""
    from eagleeverything_amd import rcpp_api
    n = 203
    Mt8 = planted_panel(n, L, 200 + L)
    fMt = write_pair(tmp_path, Mt8)
    for P in (1, 3):
        check(fMt, Mt8, planted_trait(n, P, L + P), seed=L, R=40)
    rcpp_api.drop_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129])
def test_gpu_maxt_every_R(tmp_path, R):
    """The 32-permutation operand block and the workgroup's permutation width (128 with one plane, 64 with two or three) and one either
    side of each, from the first ordinal and from the millionth."""
    from eagleeverything_amd import rcpp_api
    n, L = 203, 129
    Mt8 = planted_panel(n, L, 300 + R)
    fMt = write_pair(tmp_path, Mt8)
    for P, first in ((1, 1), (2, 1000000), (3, 1), (1, 1000000)):
        check(fMt, Mt8, planted_trait(n, P, R + P), seed=R + 5, first=first, R=R)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 2. used, strata, explicit permutations
@pytest.mark.gpu
def test_gpu_maxt_used_strata_and_explicit_permutations(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    rng = np.random.default_rng(3)
    n, L, R = 400, 150, 37
    Mt8 = planted_panel(n, L, 7)
    fMt = write_pair(tmp_path, Mt8)
    used = rng.random(n) < 0.8
    used[128:256] = False                                                  # a whole chunk of 128 individuals without a used one
    used[[0, 127, 256, n - 1]] = True
    strata = rng.integers(0, 5, n) * 13107                                 # strata 0 .. 52428
    strata[n - 1] = 65535
    strata[0] = 65535
    for P in (1, 2, 3):
        t = planted_trait(n, P, 40 + P)
        check(fMt, Mt8, t, used=used, seed=2, R=R)
        got = check(fMt, Mt8, t, used=used, strata=strata, seed=2, R=R)
        assert not np.array_equal(got["maxkey"], check(fMt, Mt8, t, strata=strata, seed=2, R=R)["maxkey"])
        # values on unused individuals are never read: beyond the limit there, and the same words
        t2 = t.copy()
        t2[~used] = 5000000
        same(rcpp_api.maxt(fMt, (n, L), t2, used=used, strata=strata, seed=2, R=R), got, "unused")
    # every used individual in its own stratum: every permutation is the identity
    own = check(fMt, Mt8, t, used=used, strata=np.arange(n), seed=9, R=6)
    assert np.array_equal(own["count1"], np.full(L, 6)) and np.all(own["maxkey"] == own["key_obs"].max())
    assert np.all(own["argmax"] == int(np.argmax(own["key_obs"])))
    # the explicit route: the identity, a reversal, random rows; and the seeded rows handed over explicitly give the seeded call's words
    N = int(used.sum())
    perm = np.stack([np.arange(N), np.arange(N)[::-1]] + [rng.permutation(N) for _ in range(4)])
    ex = check(fMt, Mt8, t, used=used, strata=strata, seed=77, R=6, perm=perm)
    assert ex["maxkey"][0] == ex["key_obs"].max() and np.all(ex["count1"] >= 1)
    rows = r_api.maxt_permutations_host(N, strata[used], 2, 1, R)
    same(rcpp_api.maxt(fMt, (n, L), t, used=used, R=R, perm=rows), got, "seeded rows as perm")
    with pytest.raises(rcpp_api.EagleError):
        rcpp_api.maxt(fMt, (n, L), t, used=used, R=1, perm=np.zeros((1, N), dtype=np.int64))
    rcpp_api.drop_cache()


@pytest.mark.gpu
def test_gpu_maxt_split_invariance(tmp_path):
    """Calls over [1, a] and [a + 1, R] add up to the call over [1, R]; more than EAGLE_MAXT_RMAX permutations run as several calls."""
    from eagleeverything_amd import rcpp_api
    n, L, R = 150, 140, 1030
    Mt8 = planted_panel(n, L, 11)
    fMt = write_pair(tmp_path, Mt8)
    t = planted_trait(n, 2, 5)
    strata = np.arange(n) % 4
    whole = check(fMt, Mt8, t, strata=strata, seed=123, R=R)               # 1024 + 6 inside the wrapper
    a = rcpp_api.maxt(fMt, (n, L), t, strata=strata, seed=123, first=1, R=70)
    b = rcpp_api.maxt(fMt, (n, L), t, strata=strata, seed=123, first=71, R=R - 70)
    assert np.array_equal(a["count1"] + b["count1"], whole["count1"])
    assert np.array_equal(np.concatenate([a["maxkey"], b["maxkey"]]).view(np.uint64), whole["maxkey"].view(np.uint64))
    assert np.array_equal(np.concatenate([a["argmax"], b["argmax"]]), whole["argmax"])
    for k in ("d_obs", "V", "key_obs"):
        assert np.array_equal(a[k], whole[k]) and np.array_equal(b[k], whole[k])
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 3. the sort's paths and the capacity
@pytest.mark.gpu
@pytest.mark.parametrize("n,L,R", [(2048, 20, 3), (2049, 20, 3), (5000, 30, 5), (65535, 64, 4), (65535, 8, 260)])
def test_gpu_maxt_long_permutations(tmp_path, n, L, R):
    """One bitonic chunk in LDS (2,048 keys), the first size with steps in global memory, three levels of them, and the capacity of the
    16-bit index: 65,535 individuals, where a key block of 256 permutations makes R = 260 two blocks."""
    from eagleeverything_amd import rcpp_api
    Mt8 = planted_panel(n, L, n % 1000)
    fMt = write_pair(tmp_path, Mt8)
    strata = None if n == 2048 else np.arange(n) % 3
    check(fMt, Mt8, planted_trait(n, 3, n % 97), strata=strata, seed=2 ** 64 - 3, first=1000000, R=R)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 4. routes
@pytest.mark.gpu
def test_gpu_maxt_resident_streamed_text_and_view(golden, tmp_path, monkeypatch):
    from eagleeverything_amd import r_api, rcpp_api
    import os
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    Mt8 = np.ascontiguousarray(M8.T)
    rng = np.random.default_rng(1)
    t = planted_trait(n, 3, 9)
    used = rng.random(n) < 0.9
    strata = rng.integers(0, 3, n)
    R = 70
    want = r_api.maxt_host(Mt8, t, used, strata, 4, 1, R)
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    fMt = geno["asciifileMt"]
    args = dict(used=used, strata=strata, seed=4, first=1, R=R)
    same(rcpp_api.maxt(fMt, (n, L), t, **args), want, "resident")          # the image the converter left resident
    whole = rcpp_api.marker_counts(fMt, (n, L))
    rcpp_api.drop_cache()                                                  # from the sidecar, made resident
    assert os.path.exists(fMt + ".e2b")
    same(rcpp_api.maxt(fMt, (n, L), t, **args), want, "sidecar")
    assert np.array_equal(rcpp_api.marker_counts(fMt, (n, L)), whole)      # the cached image was read, not written
    rcpp_api.drop_cache()                                                  # in row windows of 256 markers (test_gpu_marker_qc's settings)
    n_pad = (n + 255) // 256 * 256
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr((256 * n_pad - 16) / 1e9))
    same(rcpp_api.maxt(fMt, (n, L), t, **args), want, "windows")
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")                           # the same windows from the text
    same(rcpp_api.maxt(fMt, (n, L), t, **args), want, "text")
    monkeypatch.delenv("EAGLE_HIP_SIDECAR")
    monkeypatch.delenv("EAGLE_HIP_MAX_RESIDENT_GB")
    rcpp_api.drop_cache()
    # a VIEW alias: one trait record, mask entry and stratum per KEPT individual
    na = np.array([1, 2, 57, 130, 203])                                    # 1-based, as R hands them over
    kept = np.setdiff1d(np.arange(n), na - 1)
    dims = r_api.ReshapeM(geno["asciifileM"], geno["asciifileMt"], na, (n, L), view=True)
    assert dims[0] == n - 5
    wantv = r_api.maxt_host(np.ascontiguousarray(Mt8[:, kept]), t[kept], used[kept], strata[kept], 4, 1, R)
    argv = dict(used=used[kept], strata=strata[kept], seed=4, first=1, R=R)
    same(rcpp_api.maxt(fMt + "tmp", (n - 5, L), t[kept], **argv), wantv, "view")
    rcpp_api.drop_cache()                                                  # the same alias from the source's sidecar, in windows
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr(2 * 256 * 256 / 1e9))
    same(rcpp_api.maxt(fMt + "tmp", (n - 5, L), t[kept], **argv), wantv, "view in windows")
    with pytest.raises(ValueError):
        rcpp_api.maxt(fMt + "tmp", (n - 5, L), t, R=R)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 5. end to end
@pytest.mark.gpu
def test_gpu_maxt_end_to_end(tmp_path):
    """r_api.MaxT through the device equals the same statistics built from the numpy restatement, its trend chi-square is CaseControl's,
    a planted marker is never reached by a permutation's maximum, and strata of one individual freeze the trait."""
    from eagleeverything_amd import r_api, rcpp_api, synth
    rng = np.random.default_rng(21)
    n, L, R = 257, 300, 200
    Mt8 = planted_panel(n, L, 21)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    liab = 2.5 * Mt8[17] + rng.standard_normal(n)
    status = (liab > 0).astype(object)
    status[[0, 50]] = None
    status[60] = float("nan")
    pop = np.array(["a", "b", "c"])[np.arange(n) % 3]
    for within in (None, pop):
        res = r_api.MaxT(geno, status, R=R, seed=5, within=within)
        t, used, strata, kind, scale = r_api.maxt_trait(status, within)
        want = r_api.maxt_from_raw(r_api.maxt_host(Mt8, t, used, strata, 5, 1, R), t[used], kind, scale)
        assert set(res) == set(want) and res["kind"] == "cc" and res["n_used"] == n - 3 and res["R"] == R
        for k in want:
            if isinstance(want[k], np.ndarray):
                assert res[k].dtype == want[k].dtype and np.array_equal(res[k], want[k], equal_nan=True), k
            else:
                assert res[k] == want[k], k
        cc = r_api.CaseControl(geno, status)
        ok = np.arange(L) != L - 1
        assert np.all(np.abs(res["stat"][ok] - cc["trend"][ok]) <= 1e-12 * cc["trend"][ok])
        assert np.isnan(res["stat"][L - 1]) and np.isnan(res["emp1"][L - 1]) and np.isnan(res["emp2"][L - 1])
        assert np.all(res["emp2"][ok] >= res["emp1"][ok]) and res["count2"][17] == 0 and res["emp2"][17] == 1.0 / (R + 1)
    # a quantitative trait with NaN records, continued by a second call and merged
    y = 0.8 * Mt8[40] + rng.standard_normal(n)
    y[[3, 99]] = np.nan
    a, b = r_api.MaxT(geno, y, R=60, seed=8), r_api.MaxT(geno, y, R=40, seed=8, first=61)
    m, w = r_api.maxt_merge(a, b), r_api.MaxT(geno, y, R=100, seed=8)
    assert w["kind"] == "qt" and m["R"] == 100
    for k in ("count1", "count2", "emp1", "emp2", "max_stat", "argmax", "stat", "p", "beta"):
        assert np.array_equal(m[k], w[k], equal_nan=True), k
    frozen = r_api.MaxT(geno, y, R=7, seed=8, within=np.arange(n))
    assert np.array_equal(frozen["count1"], np.full(L, 7))
    rcpp_api.drop_cache()
