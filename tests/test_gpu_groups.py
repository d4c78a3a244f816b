"""Per-group genotype counts and Fisher's exact test on the GPU: eagle_group_counts (k_group_onehot, k_group_tile<1|2>),
eagle_bed_group_counts (k_group_bedmask, k_bed_group_counts), eagle_fisher_2x2 (k_fisher_2x2) and the r_api interface on top.

Expected values: r_api.group_counts_host / bed_group_counts_host / fisher_2x2_host, which tests/test_groups_host.py holds to loops over
individuals and to exact fractions on the CPU, and plain numpy counting written here.  Counts are integers and the Fisher walk has a
fixed order of correctly rounded operations: every comparison is ==."""
import os

import numpy as np
import pytest

import group_truth as truth
from test_gpu_marker_qc import ingest_text, np_counts

KS = [1, 2, 3, 31, 32, 33, 64]


def planted_labels(n, K, seed):
    """Random labels with a tenth of the individuals in no group, and planted: with K >= 3 group 1 is empty and group 2 is the single
    individual n - 1; with at least two other groups the individuals on either side of every multiple of 16 (so of 32 and 128 too) lie
    in different groups."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, K, n)
    lab[rng.random(n) < 0.1] = -1
    free = [k for k in range(K) if K < 3 or k not in (1, 2)]
    if K >= 3:
        lab[(lab == 1) | (lab == 2)] = 0
    if len(free) >= 2:
        for b in range(16, n, 16):
            lab[b - 1], lab[b] = free[(b // 16) % len(free)], free[(b // 16 + 1) % len(free)]
    if K >= 3:
        lab[n - 1] = 2
    return lab.astype(np.int32)


def planted_panel(n, L, seed):
    from eagleeverything_amd import synth
    Mt8 = synth.genotypes_marker_major(n, L, seed=seed)
    for r, v in enumerate((-1, 0, 1)):                                 # all-(-1), all-0 and all-(+1) marker rows
        if r < L:
            Mt8[L - 1 - r] = v
    return Mt8


def np_group_counts(Mt8, labels, K):
    """(L, K, 3) by counting: no matrix product, no (s, q) algebra."""
    out = np.zeros((Mt8.shape[0], K, 3), dtype=np.int32)
    for k in range(K):
        sub = Mt8[:, labels == k]
        out[:, k] = np.stack([np.sum(sub == v, axis=1) for v in (-1, 0, 1)], axis=1)
    return out


def check_all_K(fMt, n, L, Mt8, seed):
    from eagleeverything_amd import r_api, rcpp_api
    for K in KS:
        lab = planted_labels(n, K, seed + K)
        want = np_group_counts(Mt8, lab, K)
        assert np.array_equal(want, r_api.group_counts_host(Mt8, lab, K))
        if K >= 3:
            assert not want[:, 1].any() and np.array_equal(want[:, 2].sum(axis=1), np.ones(L))
        got = rcpp_api.group_counts(fMt, (n, L), lab, K)
        assert got.dtype == np.int32 and got.shape == (L, K, 3) and np.array_equal(got, want), (n, L, K)
    assert not rcpp_api.group_counts(fMt, (n, L), np.full(n, -1), 33).any()                     # nobody in a group
    whole = rcpp_api.marker_counts(fMt, (n, L))
    assert np.array_equal(rcpp_api.group_counts(fMt, (n, L), np.zeros(n), 1)[:, 0], whole)      # K = 1, all labels 0, is marker_counts
    lab = np.arange(n) % 64
    assert np.array_equal(rcpp_api.group_counts(fMt, (n, L), lab, 64).sum(axis=1), whole)       # a partition sums to it


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 257, 1003])
def test_gpu_group_counts_every_n(tmp_path, n):
    """The 16-byte piece, the MFMA k-step of 32 and the 128-byte chunk, at L = 300 (three tiles, the last of 44 markers)."""
    from eagleeverything_amd import rcpp_api, synth
    L = 300
    Mt8 = planted_panel(n, L, 100 + n)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    check_all_K(geno["asciifileMt"], n, L, Mt8, n)
    rcpp_api.drop_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 31, 33, 127, 128, 129])
def test_gpu_group_counts_every_L(tmp_path, L):
    """The 32-row block and the 128-marker tile, at n = 203."""
    from eagleeverything_amd import rcpp_api, synth
    n = 203
    Mt8 = planted_panel(n, L, 200 + L)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    check_all_K(geno["asciifileMt"], n, L, Mt8, L)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 2. routes
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["genoDemo_150x4998", "synth_203x1531"])
def test_gpu_group_counts_resident_streamed_text(golden, tmp_path, monkeypatch, case):
    from eagleeverything_amd import rcpp_api
    M8 = golden(case)["M8"]
    n, L = M8.shape
    Mt8 = np.ascontiguousarray(M8.T)
    labs = {K: planted_labels(n, K, 7 * K) for K in (5, 40)}
    truth_ = {K: np_group_counts(Mt8, labs[K], K) for K in labs}
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    fMt = geno["asciifileMt"]
    mmt = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L))
    whole = rcpp_api.marker_counts(fMt, (n, L))
    for K in labs:                                                     # the image the converter left resident
        assert np.array_equal(rcpp_api.group_counts(fMt, (n, L), labs[K], K), truth_[K])
    # the cached images were read, not written: the passes before give the bits they gave
    assert np.array_equal(rcpp_api.marker_counts(fMt, (n, L)), whole) and np.array_equal(whole, np_counts(M8))
    assert np.array_equal(rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L)), mmt)
    rcpp_api.drop_cache()                                              # from the sidecar, made resident
    assert os.path.exists(fMt + ".e2b")
    assert np.array_equal(rcpp_api.group_counts(fMt, (n, L), labs[40], 40), truth_[40])
    rcpp_api.drop_cache()                                              # in row windows of 256 markers (test_gpu_marker_qc's settings)
    n_pad = (n + 255) // 256 * 256
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr((256 * n_pad - 16) / 1e9))
    for K in labs:
        assert np.array_equal(rcpp_api.group_counts(fMt, (n, L), labs[K], K), truth_[K])
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")                       # the same windows from the text
    for K in labs:
        assert np.array_equal(rcpp_api.group_counts(fMt, (n, L), labs[K], K), truth_[K])
    rcpp_api.drop_cache()


@pytest.mark.gpu
def test_gpu_group_counts_on_view_alias(golden, tmp_path, monkeypatch):
    from eagleeverything_amd import r_api, rcpp_api
    M8 = golden("synth_203x1531")["M8"]
    n, L = M8.shape
    rcpp_api.drop_cache()
    geno = ingest_text(tmp_path, "p", M8)
    na = np.array([1, 2, 57, 130, 203])                                # 1-based, as R hands them over
    kept = np.setdiff1d(np.arange(n), na - 1)
    dims = r_api.ReshapeM(geno["asciifileM"], geno["asciifileMt"], na, (n, L), view=True)
    assert dims[0] == n - 5
    lab = planted_labels(n - 5, 33, 3)                                 # one label per KEPT individual
    want = np_group_counts(np.ascontiguousarray(M8[kept].T), lab, 33)
    assert np.array_equal(rcpp_api.group_counts(geno["asciifileMt"] + "tmp", (n - 5, L), lab, 33), want)
    rcpp_api.drop_cache()                                              # the same alias from the source's sidecar, in windows
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr(2 * 256 * 256 / 1e9))
    assert np.array_equal(rcpp_api.group_counts(geno["asciifileMt"] + "tmp", (n - 5, L), lab, 33), want)
    with pytest.raises(ValueError):
        rcpp_api.group_counts(geno["asciifileMt"] + "tmp", (n - 5, L), planted_labels(n, 33, 3), 33)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 3. .bed
@pytest.mark.gpu
@pytest.mark.parametrize("n", [150, 203, 301, 1004])
def test_gpu_bed_group_counts(tmp_path, n):
    """n % 4 = 2, 3, 1, 0, none a multiple of 16; 5 % missing; 10, 13, 19, 63 dwords a row: G = 16, 16, 32, 64 lanes per row."""
    from eagleeverything_amd import r_api, rcpp_api, synth
    L = 333
    Mt8 = planted_panel(n, L, n)
    miss = np.random.default_rng(n).random((L, n)) < 0.05
    miss[5] = True                                                     # one marker without a single call
    miss[9] = False
    miss[9, 4 * ((n - 1) // 4):] = True                                # missing genotypes only in the last (partial) byte
    bed = synth.write_bed(str(tmp_path / "panel"), Mt8, missing=miss)
    codes = r_api.read_bed_codes(bed, (n, L))
    for K in KS:
        lab = planted_labels(n, K, n + K)
        want = np.zeros((L, K, 4), dtype=np.int32)
        for k in range(K):
            m = lab == k
            want[:, k, :3] = np.stack([np.sum((Mt8[:, m] == v) & ~miss[:, m], axis=1) for v in (-1, 0, 1)], axis=1)
            want[:, k, 3] = miss[:, m].sum(axis=1)
        assert np.array_equal(want, r_api.bed_group_counts_host(codes, lab, K))
        got = rcpp_api.bed_group_counts(bed, (n, L), lab, K)
        assert got.dtype == np.int32 and got.shape == (L, K, 4) and np.array_equal(got, want), (n, K)
        if K in (3, 64):                                               # windows of 100 rows == one window
            assert np.array_equal(rcpp_api.bed_group_counts(bed, (n, L), lab, K, max_memory_in_Gbytes=4 * 100 * ((n + 3) // 4) / 1e9), want)
    whole = rcpp_api.bed_marker_counts(bed, (n, L))
    assert np.array_equal(rcpp_api.bed_group_counts(bed, (n, L), np.zeros(n), 1)[:, 0], whole)
    assert np.array_equal(rcpp_api.bed_group_counts(bed, (n, L), np.arange(n) % 64, 64).sum(axis=1), whole)
    assert not rcpp_api.bed_group_counts(bed, (n, L), np.full(n, -1), 7).any()
    # without a missing code the first three columns are the image route's
    rcpp_api.drop_cache()
    full = synth.write_bed(str(tmp_path / "full"), Mt8)
    d = tmp_path / "txt"
    d.mkdir()
    geno = synth.write_geno_pair(str(d), Mt8)
    lab = planted_labels(n, 33, 1)
    b = rcpp_api.bed_group_counts(full, (n, L), lab, 33)
    assert not b[:, :, 3].any() and np.array_equal(b[:, :, :3], rcpp_api.group_counts(geno["asciifileMt"], (n, L), lab, 33))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 4. more than 64 groups
@pytest.mark.gpu
def test_gpu_more_than_64_groups_in_rounds(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L, K = 1003, 150, 130
    Mt8 = planted_panel(n, L, 9)
    lab = planted_labels(n, K, 9)
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    got = rcpp_api.group_counts(geno["asciifileMt"], (n, L), lab, K)
    assert got.shape == (L, K, 3) and np.array_equal(got, np_group_counts(Mt8, lab, K))
    assert np.array_equal(rcpp_api.group_counts(geno["asciifileMt"], (n, L), lab)[:, :K], got[:, :int(lab.max()) + 1])    # K from the labels
    bed = synth.write_bed(str(tmp_path / "panel"), Mt8)
    assert np.array_equal(rcpp_api.bed_group_counts(bed, (n, L), lab, K)[:, :, :3], got)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 5. Fisher
@pytest.mark.gpu
def test_gpu_fisher_equals_the_host_walk_bit_for_bit():
    from eagleeverything_amd import r_api, rcpp_api
    t = np.array(truth.FISHER_TABLES, dtype=np.int64)
    want = r_api.fisher_2x2_host(t)
    got = rcpp_api.fisher_2x2(t)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # zero margins, N = 0, a margin of 100,000 (the legs end at their first zero term long before the margin does)
    edge = np.array([[0, 0, 0, 0], [0, 0, 5, 9], [5, 9, 0, 0], [0, 5, 0, 9], [5, 0, 9, 0], [0, 0, 0, 1], [50000, 50000, 49000, 51000],
                     [100000, 0, 0, 100000], [3, 99997, 40, 99960]], dtype=np.int64)
    want = r_api.fisher_2x2_host(edge)
    assert want[:6].tolist() == [1.0] * 6 and 0.0 <= want[7] < 1e-300 and 0.0 < want[6] < 1.0
    assert np.array_equal(rcpp_api.fisher_2x2(edge).view(np.uint64), want.view(np.uint64))
    rng = np.random.default_rng(4)
    for L in (1, 255, 257):                                            # one block, its last thread, the first thread of a second block
        tabs = rng.integers(0, 60, (L, 4))
        assert np.array_equal(rcpp_api.fisher_2x2(tabs).view(np.uint64), r_api.fisher_2x2_host(tabs).view(np.uint64))


# ------------------------------------------------------------------------------------------------ 6. end to end
@pytest.mark.gpu
def test_gpu_fst_and_case_control_end_to_end(tmp_path):
    """A two-population panel (allele frequencies drawn apart, Balding-Nichols style): Fst, GroupCounts and CaseControl through the
    device equal the same functions fed the numpy restatement of the counts."""
    from eagleeverything_amd import r_api, rcpp_api, synth
    rng = np.random.default_rng(21)
    n, L = 257, 400
    pop = np.array(["north", "south"])[(np.arange(n) >= 120).astype(int)].astype(object)
    pop[[3, 200]] = None                                               # two individuals of no population
    anc = rng.uniform(0.1, 0.9, L)
    f = np.stack([rng.beta(anc * 4, (1 - anc) * 4) for _ in range(2)], axis=1)       # Fst about 0.2
    which = (np.arange(n) >= 120).astype(int)
    Mt8 = (rng.random((L, n)) < f[:, which]).astype(np.int8) + (rng.random((L, n)) < f[:, which]).astype(np.int8) - 1
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    lab, names = r_api.group_labels(pop)
    assert names == ["north", "south"] and (lab == -1).sum() == 2
    host = r_api.group_counts_host(Mt8, lab, 2)
    gc = r_api.GroupCounts(geno, pop)
    assert gc["names"] == names and np.array_equal(gc["counts"], host) and gc["sizes"].tolist() == [119, 136]
    st = r_api.marker_stats_from_counts(host[:, 1, 0], host[:, 1, 1], host[:, 1, 2])
    assert np.array_equal(gc["freq"][:, 1], st["freq"], equal_nan=True) and np.array_equal(gc["maf"][:, 1], st["maf"], equal_nan=True)
    inc = np.arange(0, L, 3)
    assert np.array_equal(r_api.GroupCounts(geno, pop, include=inc)["counts"], host[inc])
    assert np.array_equal(r_api.HWE(gc["counts"][:, 0]), r_api.HWE(host[:, 0]))
    chrom = {"Chr": np.repeat(["1", "2"], L // 2), "Pos": np.tile(np.arange(L // 2) * 1000 + 1, 2)}
    for method in ("hudson", "wc"):
        a = r_api.Fst(geno, pop, method=method, map=chrom, window=50)
        b = r_api.fst_from_counts(host, method=method, chrom=np.repeat([0, 1], L // 2), window=50)
        assert a.pop("names") == names and set(a) == set(b)
        for k in b:
            if k == "windows":
                assert all(np.array_equal(a[k][j], b[k][j], equal_nan=True) for j in b[k])
            else:
                assert np.array_equal(a[k], b[k], equal_nan=True), (method, k)
    assert 0.05 < r_api.Fst(geno, pop)["genome"][0] < 0.5
    status = rng.integers(0, 2, n).astype(object)
    status[[0, 50]] = None
    status[60] = float("nan")
    sl = np.array([-1 if (v is None or v != v) else int(v) for v in status], dtype=np.int32)
    cc = r_api.CaseControl(geno, status, fisher=True)
    want = r_api.case_control_from_counts(r_api.group_counts_host(Mt8, sl, 2), fisher=r_api.fisher_2x2_host)
    assert set(cc) == set(want) and "p_fisher" in cc
    for k in want:
        assert np.array_equal(np.asarray(cc[k]).view(np.uint64) if cc[k].dtype == np.float64 else cc[k],
                              np.asarray(want[k]).view(np.uint64) if want[k].dtype == np.float64 else want[k]), k
    # the .bed route without a missing code gives the same tests
    synth.write_bed(str(tmp_path / "panel"), Mt8)
    cb = r_api.CaseControl(geno, status, bed=str(tmp_path / "panel"))
    assert all(np.array_equal(cb[k], want[k], equal_nan=True) for k in cb)
    rcpp_api.drop_cache()
