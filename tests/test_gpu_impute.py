"""kNN imputation on the GPU: eagle_knn_rows / eagle_bed_impute_knn (k_knn_rows, k_bed_impute on the hot paths) and ImputeBed /
ReadMarker(impute=) on top.

The device's output file and counts are compared with r_api.impute_knn_host, the neighbour table with r_api.knn_rows_host -- the
numpy restatements that tests/test_impute_host.py pins to plain loops of the definitions.  Files are bytes and counts are integers:
every comparison is ==."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEAD = b"\x6c\x1b\x01"


def make_panel(n, L, seed, rate=0.15):
    """(Mt8, missing) of a random panel with the planted rows the shapes allow."""
    rng = np.random.default_rng(seed)
    Mt8 = rng.integers(-1, 2, size=(L, n)).astype(np.int8)
    miss = rng.random((L, n)) < rate
    if L >= 3:
        miss[0, :] = True                    # a marker with every genotype missing
        miss[1, :] = False                   # a marker with none missing
        miss[2, : max(1, n - 1)] = True      # all of individual 0's possible neighbours but the last are missing here
    return Mt8, miss


def table(n, K, seed):
    """A neighbour table of knn_rows' shape (distinct others in a random order, then -1) without the cost of making distances."""
    rng = np.random.default_rng(seed)
    nbr = np.full((n, K), -1, dtype=np.int32)
    keff = min(K, n - 1)
    if keff:
        for i in range(n):
            p = rng.permutation(n - 1)[:keff]
            nbr[i, :keff] = p + (p >= i)
    return nbr


def check_against_host(tmp_path, n, L, nbr, k, min_votes, seed, mem=8.0, tag=""):
    from eagleeverything_amd import r_api, rcpp_api, synth
    Mt8, miss = make_panel(n, L, seed)
    bed = synth.write_bed(str(tmp_path / ("in%s" % tag)), Mt8, missing=miss)
    before = open(bed, "rb").read()
    out = str(tmp_path / ("out%s.bed" % tag))
    counts = rcpp_api.bed_impute_knn(bed, (n, L), nbr, k, min_votes, out, max_memory_in_Gbytes=mem)
    want_rows, want_counts = r_api.impute_knn_host(r_api.read_bed_codes(bed, (n, L)), nbr, k, min_votes)
    got = open(out, "rb").read()
    assert got == HEAD + want_rows.tobytes()
    assert counts.dtype == np.int32 and counts.shape == (L, 2) and np.array_equal(counts, want_counts)
    assert open(bed, "rb").read() == before                                   # the input is only read
    return bed, out, counts, miss


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257, 1003])
@pytest.mark.parametrize("L", [1, 17, 300])
def test_gpu_bed_impute_equals_host(tmp_path, n, L):
    from eagleeverything_amd import rcpp_api
    K = {1: 1, 3: 2, 4: 7, 5: 4, 63: 62, 64: 64, 65: 16, 257: 256, 1003: 32}[n]     # K = 1, n - 1, > n - 1 (a -1 tail), the largest
    k = {1: 1, 3: 1, 4: 7, 5: 2, 63: 5, 64: 64, 65: 16, 257: 10, 1003: 5}[n]        # k = K among them
    nbr = table(n, K, seed=n)
    bed, out, counts, miss = check_against_host(tmp_path, n, L, nbr, k, 1, seed=100 * n + L)
    mc_in = rcpp_api.bed_marker_counts(bed, (n, L))
    assert np.array_equal(counts[:, 0] + counts[:, 1], mc_in[:, 3]) and np.array_equal(mc_in[:, 3], miss.sum(axis=1))
    mc_out = rcpp_api.bed_marker_counts(out, (n, L))
    assert not np.any(mc_out[:, 3]) and np.array_equal(mc_out[:, :3].sum(axis=1), np.full(L, n))
    if L >= 3:
        assert counts[0].tolist() == [0, n]                                   # no call at all: every genotype by fallback ...
        rb = (n + 3) // 4
        raw = np.frombuffer(open(out, "rb").read(), dtype=np.uint8)[3:].reshape(L, rb)
        assert mc_out[0].tolist() == [0, n, 0, 0]                             # ... and heterozygous
        src = np.frombuffer(open(bed, "rb").read(), dtype=np.uint8)[3:].reshape(L, rb)
        assert counts[1].tolist() == [0, 0] and np.array_equal(raw[1], src[1])   # nothing missing: the row itself (its pad bits are 00)


def test_gpu_bed_impute_clears_pad_bits(tmp_path):
    """A file whose unused bit pairs are not zero (PLINK never writes one, but nothing forbids it): they go out as 00."""
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L = 5, 4
    rng = np.random.default_rng(2)
    Mt8, miss = rng.integers(-1, 2, size=(L, n)).astype(np.int8), rng.random((L, n)) < 0.3
    miss[3, :] = False
    bed = synth.write_bed(str(tmp_path / "pad"), Mt8, missing=miss)
    raw = bytearray(open(bed, "rb").read())
    for m in range(L):
        raw[3 + 2 * m + 1] |= 0b01101100                                      # fields 5 .. 7 of the last byte: het, hom A2, missing
    open(bed, "wb").write(bytes(raw))
    nbr = table(n, 4, seed=1)
    out = str(tmp_path / "padout.bed")
    counts = rcpp_api.bed_impute_knn(bed, (n, L), nbr, 2, 1, out)
    codes = np.array([0, 2, 3], dtype=np.uint8)[Mt8 + 1]
    codes[miss] = 1
    rows, want = r_api.impute_knn_host(codes, nbr, 2, 1)
    assert open(out, "rb").read() == HEAD + rows.tobytes() and np.array_equal(counts, want)
    assert np.array_equal(counts.sum(axis=1), miss.sum(axis=1))               # the pad's missing code is not counted


@pytest.mark.parametrize("min_votes", [1, 3, 1000])
def test_gpu_bed_impute_fallback_rules(tmp_path, min_votes):
    """Listed neighbours that are all missing at a marker, and min_votes above the voters there are: the marker's own mean."""
    from eagleeverything_amd import synth, rcpp_api
    n, L, K = 65, 17, 3
    nbr = table(n, K, seed=9)
    Mt8, miss = make_panel(n, L, seed=77, rate=0.1)
    miss[5, :] = False
    miss[5, 0] = True
    miss[5, nbr[0]] = True                                                    # individual 0 and its three neighbours: missing at marker 5
    Mt8[5, ~miss[5]] = 1                                                      # every call there is hom A2: so is the fallback
    bed = synth.write_bed(str(tmp_path / "fb"), Mt8, missing=miss)
    from eagleeverything_amd import r_api
    out = str(tmp_path / "fbout.bed")
    counts = rcpp_api.bed_impute_knn(bed, (n, L), nbr, K, min_votes, out)
    rows, want = r_api.impute_knn_host(r_api.read_bed_codes(bed, (n, L)), nbr, K, min_votes)
    assert open(out, "rb").read() == HEAD + rows.tobytes() and np.array_equal(counts, want)
    assert counts[5, 1] >= 1 and (rows[5, 0] & 3) == 3                        # individual 0 at marker 5: by fallback, hom A2
    if min_votes > K:
        assert not np.any(counts[:, 0]) and np.array_equal(counts[:, 1], miss.sum(axis=1))
    if min_votes == 1:
        assert counts[5].tolist()[1] <= 4


def test_gpu_bed_impute_windows_give_the_same_bytes(tmp_path):
    from eagleeverything_amd import rcpp_api
    n, L = 257, 300
    nbr = table(n, 16, seed=4)
    mem = 4 * 50 * ((n + 3) // 4) / 1e9                                        # staging windows of 50 rows: six of them
    _, one, c_one, _ = check_against_host(tmp_path, n, L, nbr, 5, 1, seed=12, tag="a")
    _, many, c_many, _ = check_against_host(tmp_path, n, L, nbr, 5, 1, seed=12, mem=mem, tag="b")
    assert open(one, "rb").read() == open(many, "rb").read() and np.array_equal(c_one, c_many)


def test_gpu_bed_impute_refuses_and_leaves_no_file(tmp_path):
    from eagleeverything_amd import rcpp_api, synth
    n, L = 9, 5
    Mt8, miss = make_panel(n, L, seed=1)
    bed = synth.write_bed(str(tmp_path / "r"), Mt8, missing=miss)
    out = str(tmp_path / "rout.bed")
    nbr = table(n, 4, seed=1)
    for kw in (dict(k=5), dict(k=0), dict(min_votes=0), dict(out=bed), dict(dims=(n, L + 1))):
        with pytest.raises(rcpp_api.EagleError):
            rcpp_api.bed_impute_knn(bed, kw.get("dims", (n, L)), nbr, kw.get("k", 2), kw.get("min_votes", 1), kw.get("out", out))
        assert not os.path.exists(out) or os.path.getsize(out) == 0
    bad = nbr.copy()
    bad[3, 1] = n
    with pytest.raises(rcpp_api.EagleError):
        rcpp_api.bed_impute_knn(bed, (n, L), bad, 2, 1, out)
    assert not os.path.exists(out)


@pytest.mark.parametrize("n", [1, 2, 5, 256, 257, 1003])
def test_gpu_knn_rows_equals_host(n):
    from eagleeverything_amd import r_api, rcpp_api
    rng = np.random.default_rng(n)
    G = rng.integers(-1, 2, size=(n, 24)).astype(np.int64)                    # 24 markers: d <= 96, ties everywhere
    if n >= 5:
        G[3] = G[1]                                                           # a duplicate pair: distance 0
        G[4] = G[1]
    ibs0 = (G @ G.T - (G * G) @ (G * G).T) // -2                              # (Q - D) / 2
    hethet = (1 - G * G) @ (1 - G * G).T
    ibs0, hethet = ibs0.astype(np.int32), hethet.astype(np.int32)
    d = r_api.knn_distance(ibs0, hethet)
    assert np.array_equal(d[0], ((G[0][None, :] - G) ** 2).sum(axis=1))
    for K in sorted({1, 7, max(1, min(n - 1, 256)), min(n + 2, 256), 256}):
        got = rcpp_api.knn_rows(ibs0, hethet, K)
        assert got.dtype == np.int32 and got.shape == (n, K)
        assert np.array_equal(got, r_api.knn_rows_host(d, K))
    if n >= 5:
        assert got[1, :2].tolist() == [3, 4] and got[3, :2].tolist() == [1, 4]


def test_gpu_knn_rows_planted_ties_in_a_hand_made_matrix():
    """Not a distance of any panel: rows of one value (index order alone decides) and large values next to small ones."""
    from eagleeverything_amd import r_api, rcpp_api
    n = 300
    rng = np.random.default_rng(8)
    hethet = np.zeros((n, n), dtype=np.int32)                                 # h = 0: d = 4 ibs0
    ibs0 = rng.integers(0, 3, size=(n, n)).astype(np.int32)
    ibs0[0, :] = 5
    ibs0[1, :] = (1 << 29) - 1                                                # d = 2^31 - 4: the top of int32
    ibs0[2, ::2] = 0
    got = rcpp_api.knn_rows(ibs0, hethet, 40)
    assert np.array_equal(got, r_api.knn_rows_host(r_api.knn_distance(ibs0, hethet), 40))
    assert got[0].tolist() == list(range(1, 41)) and got[1].tolist() == [0] + list(range(2, 41))


def test_gpu_read_marker_impute_end_to_end(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L, k = 150, 100, 5
    rng = np.random.default_rng(21)
    founders = rng.integers(-1, 2, size=(6, L))
    M = np.repeat(founders, 25, axis=0)
    M = np.where(rng.random(M.shape) < 0.05, rng.integers(-1, 2, size=M.shape), M).astype(np.int8)
    miss = rng.random((L, n)) < 0.08
    src = tmp_path / "src"
    src.mkdir()
    bed = synth.write_bed(str(src / "panel"), np.ascontiguousarray(M.T), missing=miss)
    before = {p: open(p, "rb").read() for p in r_api.bed_fileset(bed)}
    work = tmp_path / "work"
    work.mkdir()
    said = []
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(work), impute=k, message=said.append)
    imputed = os.path.join(str(work), "imputed", "panel")
    assert geno["dim_of_ascii_M"] == [n, L]
    assert geno["asciifileM"] == os.path.join(str(work), "imputed", "M.ascii") and geno["asciifileMt"] == os.path.join(str(work), "imputed", "Mt.ascii")
    for p, ext in zip(r_api.bed_fileset(bed), (".bed", ".bim", ".fam")):
        assert open(p, "rb").read() == before[p]
        if ext != ".bed":
            assert open(imputed + ext, "rb").read() == before[p]              # .bim and .fam: byte for byte
    assert any("Imputed %d missing genotypes" % miss.sum() in s for s in said)
    stats = r_api.MarkerStats(geno, bed=imputed)
    assert not np.any(stats["n_missing"])

    # the host restatement from the original ingestion (made again, elsewhere)
    plain = tmp_path / "plain"
    plain.mkdir()
    g0 = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(plain))
    assert open(g0["asciifileM"], "rb").read() == open(os.path.join(str(work), "M.ascii"), "rb").read()
    ibs0, hethet = rcpp_api.sample_ibs(g0["asciifileM"], (n, L))
    nbr = r_api.knn_rows_host(r_api.knn_distance(ibs0, hethet), 64)
    rows, counts = r_api.impute_knn_host(r_api.read_bed_codes(bed, (n, L)), nbr, k, 1)
    assert open(imputed + ".bed", "rb").read() == HEAD + rows.tobytes()
    dec = np.stack([(rows >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(L, -1)[:, :n]
    digits = np.array([0, 9, 1, 2], dtype=np.uint8)[dec]                      # '0', '1', '2' of Mt.ascii
    text = np.concatenate([digits + ord("0"), np.full((L, 1), ord("\n"), dtype=np.uint8)], axis=1)
    assert open(geno["asciifileMt"], "rb").read() == text.tobytes()
    Mi = digits.T.astype(np.int64) - 1
    mmt = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 2, np.nan, (n, L))
    assert np.array_equal(mmt, (Mi @ Mi.T).astype(np.float64))
    assert np.mean(Mi[miss.T] == M[miss.T]) > np.mean(M[miss.T] == 0)         # better than the heterozygotes it replaces

    res = r_api.ImputeBed(bed, g0, str(tmp_path / "again" / "p"), k=k)
    assert res["n_missing"] == int(miss.sum()) == res["by_vote"] + res["by_fallback"] and np.array_equal(res["counts"], counts)
    assert open(res["bed"], "rb").read() == HEAD + rows.tobytes()
    assert r_api.ReadMarker(str(src / "panel"), type="text", AA=0, AB=1, BB=2, impute=k) is None    # impute needs a .bed file
