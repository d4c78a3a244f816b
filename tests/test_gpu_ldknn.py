"""LD-kNNi on the GPU: eagle_ld_partners (k_ld_tile's r2 mode on the int8 MFMA, k_ld_partners) and eagle_bed_impute_ldknn
(k_bed_impute_ldknn), and ImputeBed(local=) / ReadMarker(impute_local=) on top.

The device's tables, files and counts are compared with r_api.ld_partners_host and r_api.impute_ldknn_host -- the numpy restatements
that tests/test_ldknn_host.py pins to plain loops of the definitions.  Partners are integers, r2 is compared bit for bit, files are
bytes: every comparison is ==."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEAD = b"\x6c\x1b\x01"
WINDOW_L = ((1, 1), (50, 16), (256, 32), (33, 7))


# ------------------------------------------------------------------------------------------------ partners
def partner_panel(n, L, seed):
    """Random genotypes with what the shapes allow: identical markers across the 128-marker tile edge and the 32-row block edge (ties in
    r2, seen from one side and from both), monomorphic markers beside those edges."""
    from eagleeverything_amd import synth
    Mt8 = synth.genotypes_marker_major(n, L, seed=seed)
    if L >= 129:
        Mt8[127] = Mt8[128] = Mt8[124]
        Mt8[126] = 1
        Mt8[31] = Mt8[33] = Mt8[32]
        Mt8[30] = 0
    if L >= 300:
        Mt8[255] = Mt8[256] = Mt8[258]
        Mt8[257] = -1
        Mt8[299] = Mt8[297]
    return Mt8


def chrom_of(L):
    return (3 - (np.arange(L) >= 70) - (np.arange(L) >= 200)).astype(np.int32)      # 3, 2, 1: changes inside the tiles, not sorted


@pytest.mark.parametrize("n", [1, 3, 64, 65, 257])
@pytest.mark.parametrize("L", [1, 2, 129, 300])
def test_gpu_ld_partners_equals_host(tmp_path, n, L):
    from eagleeverything_amd import r_api, rcpp_api, synth
    Mt8 = partner_panel(n, L, seed=1000 * n + L)
    Mt = str(tmp_path / "Mt.ascii")
    synth.write_ascii(Mt, Mt8)
    rcpp_api.drop_cache()
    for window, l in WINDOW_L:
        for chrom, min_r2 in ((None, 0.0), (chrom_of(L), 0.0), (None, 0.05)):
            want, want_r2 = r_api.ld_partners_host(Mt8, window, l, min_r2, chrom)
            got, got_r2 = rcpp_api.ld_partners(Mt, (n, L), window, l, min_r2, chrom, return_r2=True)
            assert got.dtype == np.int32 and got.shape == (L, l) and got_r2.dtype == np.float64
            assert np.array_equal(got, want), (window, l, min_r2, np.flatnonzero((got != want).any(axis=1))[:10])
            assert np.array_equal(got_r2.view(np.uint64), want_r2.view(np.uint64)), (window, l, min_r2)
            assert np.array_equal(rcpp_api.ld_partners(Mt, (n, L), window, l, min_r2, chrom), want)     # r2_out == NULL
    if n == 1:
        assert (got == -1).all()                                              # every marker is monomorphic
    if L >= 129 and n >= 64:
        got, r2 = rcpp_api.ld_partners(Mt, (n, L), 50, 16, return_r2=True)
        assert got[127, :2].tolist() == [128, 124] and got[128, :2].tolist() == [127, 124] and got[124, :2].tolist() == [127, 128]
        assert got[32, :2].tolist() == [31, 33] and r2[32, :2].tolist() == [1.0, 1.0]
        assert (got[[126, 30]] == -1).all() and not np.isin(got, [126, 30]).any()
    rcpp_api.drop_cache()


def test_gpu_ld_partners_streamed_equals_resident(tmp_path, monkeypatch):
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L = 65, 5000
    Mt8 = synth.genotypes_marker_major(n, L, seed=77)
    for a in (1500, 1791, 1792, 2047, 2048, 3400):                            # around the rows where windows of 1,792 and 2,048 rows end
        Mt8[a + 1], Mt8[a - 40], Mt8[a + 200] = Mt8[a], -Mt8[a], Mt8[a]
    Mt8[1793], Mt8[2049] = 0, 1
    chrom = (np.arange(L) >= 1800).astype(np.int32)
    path = str(tmp_path / "Mt.ascii")
    synth.write_ascii(path, Mt8)
    want = {(w, l): r_api.ld_partners_host(Mt8, w, l, 0.0, chrom) for w, l in ((50, 16), (256, 32))}
    rcpp_api.drop_cache()
    for (w, l), (p, r2) in want.items():
        got, got_r2 = rcpp_api.ld_partners(path, (n, L), w, l, 0.0, chrom, return_r2=True)
        assert np.array_equal(got, p) and np.array_equal(got_r2.view(np.uint64), r2.view(np.uint64))
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.001")                  # 1 MB: the 5,120 x 256 image goes in at least 3 row windows
    for (w, l), (p, r2) in want.items():
        got, got_r2 = rcpp_api.ld_partners(path, (n, L), w, l, 0.0, chrom, return_r2=True)
        assert np.array_equal(got, p), (w, l, np.flatnonzero((got != p).any(axis=1))[:10])
        assert np.array_equal(got_r2.view(np.uint64), r2.view(np.uint64))
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ imputation
def make_bed(tmp_path, n, L, seed, rate=0.2, tag=""):
    """A fileset with `rate` missing, the planted rows the shapes allow, and the pad bit pairs of every row's last byte set to garbage."""
    from eagleeverything_amd import synth
    rng = np.random.default_rng(seed)
    Mt8 = rng.integers(-1, 2, size=(L, n)).astype(np.int8)
    miss = rng.random((L, n)) < rate
    if L >= 3:
        miss[0, :] = True                    # a marker with every genotype missing
        miss[1, :] = False                   # a marker with none missing
        miss[2, : max(1, n - 1)] = True      # one call at most
    bed = synth.write_bed(str(tmp_path / ("in%s" % tag)), Mt8, missing=miss)
    if n % 4:
        rb = (n + 3) // 4
        raw = bytearray(open(bed, "rb").read())
        pad = (0b01101101 << (2 * (n % 4))) & 0xff                            # missing, hom A2, het: never individuals
        for m in range(L):
            raw[3 + m * rb + rb - 1] |= pad
        open(bed, "wb").write(bytes(raw))
    return bed, miss


def partner_table(L, l, seed, span=256):
    """A table of eagle_ld_partners' shape: distinct markers within `span` rows in a random order, then -1; some rows empty."""
    rng = np.random.default_rng(seed)
    part = np.full((L, l), -1, dtype=np.int32)
    for m in range(L):
        near = np.array([j for j in range(max(0, m - span), min(L, m + span + 1)) if j != m], dtype=np.int64)
        cnt = min(near.size, int(rng.integers(0, l + 1)) if m % 7 == 3 else l)
        if cnt:
            part[m, :cnt] = rng.permutation(near)[:cnt]
    return part


def check_against_host(tmp_path, n, L, l, k, min_votes, min_overlap, seed, mem=8.0, tag="", span=256):
    from eagleeverything_amd import r_api, rcpp_api
    bed, miss = make_bed(tmp_path, n, L, seed, tag=tag)
    part = partner_table(L, l, seed + 1, span)
    before = open(bed, "rb").read()
    out = str(tmp_path / ("out%s.bed" % tag))
    counts = rcpp_api.bed_impute_ldknn(bed, (n, L), part, k, min_votes, min_overlap, out, max_memory_in_Gbytes=mem)
    want_rows, want_counts = r_api.impute_ldknn_host(r_api.read_bed_codes(bed, (n, L)), part, k, min_votes, min_overlap)
    assert open(out, "rb").read() == HEAD + want_rows.tobytes()
    assert counts.dtype == np.int32 and counts.shape == (L, 2) and np.array_equal(counts, want_counts)
    assert np.array_equal(counts.sum(axis=1), miss.sum(axis=1))               # the pad's missing code is not counted
    assert open(bed, "rb").read() == before                                   # the input is only read
    return out, counts


NS = [1, 3, 4, 5, 63, 64, 65, 257, 1003]
LS = [1, 33, 300]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("L", LS)
def test_gpu_bed_impute_ldknn_equals_host(tmp_path, n, L):
    idx = NS.index(n) + len(NS) * LS.index(L)                                 # 27 cases: every (l, k) of {1, 7, 32} x {1, 5, 64} three times
    l, k = (1, 7, 32)[idx % 3], (1, 5, 64)[(idx // 3) % 3]
    min_overlap = 1 if l == 1 else (2 if l == 7 else 4)
    out, counts = check_against_host(tmp_path, n, L, l, k, 1, min_overlap, seed=100 * n + L)
    if L >= 3:
        assert counts[0].tolist() == [0, n] and counts[1].tolist() == [0, 0]  # no call at all: by fallback; nothing missing: a copy
    if n >= 63 and L >= 33 and l > 1:
        assert counts[:, 0].sum() > 0 and counts[3:, 0].sum() > counts[3:, 1].sum()    # votes happen


@pytest.mark.parametrize("k", [1, 5, 64])
def test_gpu_bed_impute_ldknn_min_votes_above_k_is_all_fallback(tmp_path, k):
    out, counts = check_against_host(tmp_path, 65, 33, 7, k, k + 1, 1, seed=9)
    assert not counts[:, 0].any() and counts[:, 1].sum() > 0


def test_gpu_bed_impute_ldknn_windows_give_the_same_bytes(tmp_path):
    """One window; staging windows of 50 rows (six of them); one marker per window, where the halo holds ALL of a marker's partners."""
    n, L, l = 257, 300, 7
    rb = (n + 3) // 4
    outs = []
    for tag, mem in (("a", 8.0), ("b", 4 * 50 * rb / 1e9), ("c", 4 * 1 * rb / 1e9)):     # the library's arithmetic: a quarter of the budget per window
        outs.append(check_against_host(tmp_path, n, L, l, 5, 1, 2, seed=12, mem=mem, tag=tag))
    for out, counts in outs[1:]:
        assert open(out, "rb").read() == open(outs[0][0], "rb").read() and np.array_equal(counts, outs[0][1])


def test_gpu_bed_staging_ring_lives_across_calls_on_one_context(tmp_path):
    """One context: counts in windows of 100 rows (seven of them), an imputation whose one window needs larger staging buffers, so that
    the context's ring is grown between the calls, and the counts in windows of 100 rows again."""
    from eagleeverything_amd import rcpp_api
    n, L, l = 129, 700, 7
    rb = (n + 3) // 4
    small = 4 * 100 * rb / 1e9                                                # the library's arithmetic: a quarter of the budget per window
    bed, miss = make_bed(tmp_path, n, L, seed=21)
    part = partner_table(L, l, seed=22)
    rcpp_api.close_all()                                                      # a context that has staged nothing yet
    first = rcpp_api.bed_marker_counts(bed, (n, L), max_memory_in_Gbytes=small)
    counts = rcpp_api.bed_impute_ldknn(bed, (n, L), part, 5, 1, 2, str(tmp_path / "one.bed"))
    again = rcpp_api.bed_marker_counts(bed, (n, L), max_memory_in_Gbytes=small)
    assert np.array_equal(first, again) and np.array_equal(first[:, 3], miss.sum(axis=1)) and first[:, 3].sum() > 0
    rcpp_api.close_all()
    fresh = rcpp_api.bed_impute_ldknn(bed, (n, L), part, 5, 1, 2, str(tmp_path / "fresh.bed"))
    assert np.array_equal(counts, fresh) and counts.sum() == miss.sum()
    assert open(str(tmp_path / "one.bed"), "rb").read() == open(str(tmp_path / "fresh.bed"), "rb").read()


def test_gpu_bed_impute_ldknn_refuses_and_leaves_no_file(tmp_path):
    from eagleeverything_amd import rcpp_api
    n, L = 9, 300
    bed, _ = make_bed(tmp_path, n, L, seed=1)
    out = str(tmp_path / "rout.bed")
    part = partner_table(L, 4, seed=1)
    with pytest.raises(rcpp_api.EagleError):
        rcpp_api.bed_impute_ldknn(bed, (rcpp_api.LDKNN_MAX_N + 1, L), part, 5, 1, 1, out)        # n above the limit
    assert not os.path.exists(out)
    far = part.copy()
    far[10, 2] = 267
    with pytest.raises(rcpp_api.EagleError):
        rcpp_api.bed_impute_ldknn(bed, (n, L), far, 5, 1, 1, out)                                # a partner 257 rows away
    assert not os.path.exists(out)
    for kw in (dict(k=0), dict(k=65), dict(min_votes=0), dict(min_overlap=0), dict(min_overlap=33), dict(out=bed), dict(dims=(n, L + 1))):
        with pytest.raises((rcpp_api.EagleError, ValueError)):
            rcpp_api.bed_impute_ldknn(bed, kw.get("dims", (n, L)), part, kw.get("k", 2), kw.get("min_votes", 1), kw.get("min_overlap", 1),
                                      kw.get("out", out))
        assert not os.path.exists(out) or os.path.getsize(out) == 0
    far[10, 2] = 266                                                                             # 256 rows away: the limit
    counts = rcpp_api.bed_impute_ldknn(bed, (n, L), far, 5, 1, 1, out)
    assert os.path.getsize(out) == 3 + L * ((n + 3) // 4) and counts.sum() > 0


# ------------------------------------------------------------------------------------------------ end to end
def test_gpu_read_marker_impute_local_end_to_end(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    n, L, k, l = 64, 300, 5, 16
    rng = np.random.default_rng(31)
    founders = rng.integers(0, 2, size=(6, L))
    hap = lambda: np.concatenate([founders[rng.integers(6), a:a + 30] for a in range(0, L, 30)])   # noqa: E731
    Mt8 = (np.stack([hap() + hap() for _ in range(n)], axis=1) - 1).astype(np.int8)
    miss = rng.random((L, n)) < 0.08
    src = tmp_path / "src"
    src.mkdir()
    bed = synth.write_bed(str(src / "panel"), Mt8, missing=miss)
    bim = r_api.bed_fileset(bed)[1]
    lines = open(bim).read().splitlines()
    open(bim, "w").write("".join(("2" if j < 170 else "10") + ln[1:] + "\n" for j, ln in enumerate(lines)))   # two chromosomes
    before = {p: open(p, "rb").read() for p in r_api.bed_fileset(bed)}
    work = tmp_path / "work"
    work.mkdir()
    said = []
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=str(work), impute=k, impute_local=l, message=said.append)
    imputed = os.path.join(str(work), "imputed", "panel")
    assert geno["dim_of_ascii_M"] == [n, L] and geno["asciifileM"] == os.path.join(str(work), "imputed", "M.ascii")
    for p, ext in zip(r_api.bed_fileset(bed), (".bed", ".bim", ".fam")):
        assert open(p, "rb").read() == before[p]
        if ext != ".bed":
            assert open(imputed + ext, "rb").read() == before[p]
    assert any("Imputed %d missing genotypes" % miss.sum() in s and "local LD" in s for s in said)

    # the host chain: the ingested panel is the codes with missing = heterozygous
    codes = r_api.read_bed_codes(bed, (n, L))
    ingested = np.array([-1, 0, 0, 1], dtype=np.int8)[codes]
    chrom = np.where(np.arange(L) < 170, 2, 10)
    partners, _ = r_api.ld_partners_host(ingested, 50, l, 0.0, chrom)
    rows, counts = r_api.impute_ldknn_host(codes, partners, k, 1, 4)
    assert open(imputed + ".bed", "rb").read() == HEAD + rows.tobytes()
    dec = np.stack([(rows >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(L, -1)[:, :n]
    digits = np.array([0, 9, 1, 2], dtype=np.uint8)[dec]
    text = np.concatenate([digits + ord("0"), np.full((L, 1), ord("\n"), dtype=np.uint8)], axis=1)
    assert open(geno["asciifileMt"], "rb").read() == text.tobytes()
    truth = np.array([0, 2, 3], dtype=np.uint8)[Mt8 + 1]
    assert np.mean(dec[miss] == truth[miss]) > 0.7                            # 30-marker founder segments: local neighbours know

    g0 = {"asciifileM": str(work / "M.ascii"), "asciifileMt": str(work / "Mt.ascii"), "dim_of_ascii_M": [n, L]}   # the original ingestion
    res = r_api.ImputeBed(bed, g0, str(tmp_path / "again" / "p"), k=k, local=l, map=r_api.ReadBim(bim))
    assert res["n_missing"] == int(miss.sum()) == res["by_vote"] + res["by_fallback"] and np.array_equal(res["counts"], counts)
    assert np.array_equal(res["partners"], partners) and open(res["bed"], "rb").read() == HEAD + rows.tobytes()
    plain = r_api.ImputeBed(bed, g0, str(tmp_path / "plain" / "p"), k=k)      # local=None: the genome-wide rule, another file
    assert "partners" not in plain and plain["n_missing"] == res["n_missing"]
    rcpp_api.drop_cache()
