"""The marker-count-sized paths on the GPU past 65,535 rows, 262,144 lines, 2^32 bytes and at their capacities.

tests/test_gpu_regimes.py ran the n-sized kernels at every row length with 1 to 300 markers; here n stays small (2 to 1,003) and the
marker count L is what is large.  Every case first asserts the regime it is meant to run from the arithmetic restated in
tests/marker_regimes_truth.py (its docstring holds the survey of the branches of csrc/ that switch on L; tests/test_marker_regimes_host.py
pins the arithmetic to the source text), then prints it:

  a. the loaders' row bands of 65,535 (eagle_dev_decode_ascii, _encode_ascii, _pack2b, _unpack2b and the three column-gathering
     kernels of a VIEW alias), with 67,108,864 / stride rows to a staged chunk: files of 65,535 to 196,700 lines
  b. eagle_dev_tsq_argmax past its 1,024 x 256 grid: planted ties, NaN and infinities at 1 to 1,000,003 entries, and a scan from a file
  c. eagle_dev_line_scores past its chunk of 262,144 lines, and at EAGLE_SCORES_MAX_LINE with all four digit planes of 64 columns
  d. eagle_weighted_gram at EAGLE_WGRAM_MAX_MARKERS, resident and in marker windows
  e. byte offsets past 2^31 and 2^32: one panel of 7 individuals and 16,777,300 markers, and the grid-stride and banded device kernels
     called directly

Large panels repeat a base panel of P lines (P prime) along the marker axis, with planted lines around every edge: a per-marker result
equals the base panel's at m mod P bit for bit, the planted lines are checked one by one, and the base panel's results are held to
r_api's host restatements or to numpy.  Integers, bytes and fp64 bits: every comparison is ==."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import marker_regimes_truth as R

pytestmark = pytest.mark.gpu

E2B_HEADER = 64


@pytest.fixture(autouse=True)
def delete_the_files_of_a_case(tmp_path):
    """The cases write up to 200 MB a file: none of them outlives its case."""
    yield
    for root, _, files in os.walk(str(tmp_path)):
        for f in files:
            os.remove(os.path.join(root, f))


def say(**regime):
    print("regime: " + ", ".join("%s=%s" % kv for kv in regime.items()))


def _ctx():
    import torch
    from eagleeverything_amd import _lib, rcpp_api
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    return torch, lib, rcpp_api.context(0), dev, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def assert_periodic(got, base_result, planted, planted_result, what):
    """got[m] == base_result[m mod P] for every marker m but the planted ones, which equal planted_result row by row.  Compares in slabs
    of whole periods; `got` is overwritten at the planted markers."""
    P, L = base_result.shape[0], got.shape[0]
    assert got.shape[1:] == base_result.shape[1:] and got.dtype == base_result.dtype, (what, got.shape, got.dtype, base_result.dtype)
    planted = np.asarray(planted, dtype=np.int64)
    for m, want in zip(planted.tolist(), planted_result):
        assert np.array_equal(got[m], want), (what, "planted marker", m, got[m].tolist(), np.asarray(want).tolist())
    if planted.size:
        got[planted] = base_result[planted % P]
    full = L // P
    body = got[:full * P].reshape((full, P) + got.shape[1:])
    for s in range(0, full, 128):
        eq = body[s:s + 128] == base_result
        if not eq.all():
            k, r = np.argwhere(~eq.reshape(eq.shape[0], P, -1).all(axis=2))[0]
            m = (s + k) * P + r
            raise AssertionError((what, "marker", int(m), "period", int(s + k), got[m].tolist(), base_result[r].tolist()))
    tail = got[full * P:]
    assert np.array_equal(tail, base_result[:tail.shape[0]]), (what, "the last, short period")


def bits(x):
    """fp64 as int64 bit patterns with every NaN mapped to one value (a NaN's sign and payload are not the library's contract)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return np.where(np.isnan(x), np.int64(-1), x.view(np.int64))


# ================================================================================================ a. the loaders' row bands
def loader_regime(n, L):
    text, side = R.text_rows_per_chunk(n), R.sidecar_rows_per_chunk(n)
    tb, sb = R.chunk_bands(L, text), R.chunk_bands(L, side)
    wb = R.chunk_bands(L, R.mt_window_lines(n))
    if L > R.BAND_ROWS:
        assert len(tb) >= 2 and len(sb) >= 2 and len(wb) >= 2                  # a second band in the reader of either source and in the writer
        assert tb[1][0] == sb[1][0] == wb[1][0] == R.BAND_ROWS
    else:
        assert len(tb) == len(sb) == len(wb) == 1
    say(n=n, L=L, text_rows_per_chunk=text, text_chunks=-(-L // text), text_launches=len(tb), sidecar_rows_per_chunk=side,
        sidecar_launches=len(sb), writer_window=R.mt_window_lines(n), writer_launches=len(wb), last_band_rows=tb[-1][1])
    return tb


@functools.lru_cache(maxsize=1)
def loader_panel(n, L):
    base = R.base_panel(1021, n, seed=n)
    planted = R.planted_markers(L, 1021)
    Mt8 = R.periodic_lines(base, L, planted)
    Mt8.setflags(write=False)
    return Mt8, planted


LOADER_CASES = [(n, L) for n in (37, 1003) for L in (65535, 65536, 65537, 196700)]


@pytest.mark.parametrize("n,L", LOADER_CASES)
def test_gpu_loader_bands_write_and_read_back(tmp_path, monkeypatch, n, L):
    """M.ascii by numpy -> eagle_create_Mt_ascii writes Mt.ascii and its sidecar in windows of more than 65,535 lines (k_encode_ascii,
    k_pack2b) -> the image is read back resident, from the sidecar (k_unpack2b), from the text (k_decode_ascii) and through a VIEW alias
    with five individuals dropped (k_gather_cols_i8, k_unpack2b_cols, k_decode_ascii_cols).  A character outside '0'..'2' is reported in
    the last band as it is in the first."""
    from eagleeverything_amd import rcpp_api
    tb = loader_regime(n, L)
    Mt8, planted = loader_panel(n, L)
    M8 = np.ascontiguousarray(Mt8.T)
    dims = (n, L)
    fM, fMt = str(tmp_path / "M.ascii"), str(tmp_path / "Mt.ascii")
    R.text_of(M8).tofile(fM)
    rcpp_api.drop_cache()
    rcpp_api.createMt_ASCII_rcpp(fM, fMt, "text", 8.0, dims)
    want_text = R.text_of(Mt8)
    got_text = np.frombuffer(read(fMt), dtype=np.uint8)
    assert got_text.size == want_text.size
    got_text = got_text.reshape(want_text.shape)
    bad = np.flatnonzero((got_text != want_text).any(axis=1))
    assert bad.size == 0, ("Mt.ascii differs first at line", bad[:5].tolist())
    side = np.frombuffer(read(fMt + ".e2b"), dtype=np.uint8)[E2B_HEADER:]
    want_side = R.pack2b_rows(Mt8)
    assert side.size == want_side.size
    bad = np.flatnonzero((side.reshape(want_side.shape) != want_side).any(axis=1))
    assert bad.size == 0, ("Mt.ascii.e2b differs first at row", bad[:5].tolist())
    for m in planted.tolist():                                                 # the planted lines, one by one
        assert bytes(got_text[m, :n]) == bytes((R.planted_line(m, n) + 1 + ord("0")).astype(np.uint8)), m

    truth = R.counts_of(Mt8)
    edge_loci = sorted({0, 3, L - 1} | {m for r0, _ in tb for m in (r0 - 1, r0, r0 + 1) if 0 <= m < L})

    def check_image(source):
        got = rcpp_api.marker_counts(fMt, dims)
        bad = np.flatnonzero((got != truth).any(axis=1))
        assert got.dtype == np.int32 and bad.size == 0, (source, "marker_counts differs first at", bad[:5].tolist())
    check_image("resident")                                                    # the image the converter left
    for m in edge_loci:
        assert np.array_equal(rcpp_api.extract_geno_rcpp(fM, 8.0, m, dims), M8[:, m].astype(np.int32)), m
    rcpp_api.drop_cache()
    check_image("sidecar")
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")
    check_image("text")
    monkeypatch.delenv("EAGLE_HIP_SIDECAR")

    # ---- a VIEW alias: the first, the last and three more individuals dropped
    drop = np.array(sorted({0, 5, n // 2, n - 2, n - 1}), dtype=np.int64)
    kept = np.setdiff1d(np.arange(n), drop)
    vdims = (n - drop.size, L)
    vtruth = R.counts_of(Mt8[:, kept])
    rcpp_api.drop_cache()
    assert rcpp_api.ReshapeM_rcpp(fM, fMt, drop, dims, view=True) == list(vdims)

    def check_view(source, key):
        before = rcpp_api.view_load_counts()
        got = rcpp_api.marker_counts(fMt + "tmp", vdims)
        after = rcpp_api.view_load_counts()
        bad = np.flatnonzero((got != vtruth).any(axis=1))
        assert bad.size == 0, (source, "view counts differ first at", bad[:5].tolist())
        assert after[key] > before[key] and all(after[k] == before[k] for k in after if k != key), (source, before, after)
    check_view("sidecar", "sidecar")                                           # k_unpack2b_cols; leaves the alias's image resident, not the source's
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")
    check_view("text", "text")                                                 # k_decode_ascii_cols
    monkeypatch.delenv("EAGLE_HIP_SIDECAR")
    rcpp_api.drop_cache()
    check_image("sidecar, to make the source resident")
    check_view("resident", "resident")                                         # k_gather_cols_i8
    rcpp_api.drop_cache()

    # ---- a bad character: in the first band, in the last
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")
    fbad = str(tmp_path / "bad.ascii")
    want_text.tofile(fbad)
    for line in (3, L - 2):
        with open(fbad, "r+b") as f:                                           # one byte at a time: '3' in, the genotype back
            for at, ch in ((3, want_text[3, n // 2]), (L - 2, want_text[L - 2, n // 2])):
                f.seek(at * (n + 1) + n // 2)
                f.write(b"3" if at == line else bytes([ch]))
        rcpp_api.drop_cache()
        with pytest.raises(rcpp_api.EagleError) as e:
            rcpp_api.marker_counts(fbad, dims)
        assert "1 characters outside '0'..'2'" in str(e.value), (line, str(e.value))
    monkeypatch.delenv("EAGLE_HIP_SIDECAR")
    rcpp_api.drop_cache()


def ped_bytes(M8):
    """A PLINK .ped file of an n x L matrix of -1 / 0 / +1 as "A A" / "A B" / "B B", and what the converter makes of it: it codes the
    allele it meets first at a locus as allele 0, so a locus whose first individual is "B B" comes out as the 0 <-> 2 mirror image."""
    n, L = M8.shape
    head = np.frombuffer(b"f i 0 0 1 0.5", dtype=np.uint8)
    rows = np.full((n, head.size + 4 * L + 1), ord(" "), dtype=np.uint8)
    rows[:, :head.size] = head
    body = rows[:, head.size:-1].reshape(n, L, 4)
    body[:, :, 1] = np.where(M8 == 1, ord("B"), ord("A"))
    body[:, :, 3] = np.where(M8 == -1, ord("A"), ord("B"))
    rows[:, -1] = ord("\n")
    return rows.tobytes(), np.where(M8[0] == 1, -M8, M8).astype(np.int8)


@pytest.mark.parametrize("n,L", LOADER_CASES)
def test_gpu_loader_bands_converters_and_filter(tmp_path, n, L):
    """create_ascii_from_bed and filter_markers at more than 65,535 markers; at n = 37 also createM_ASCII_rcpp from a text table and
    from a PLINK .ped file (at n = 1,003 those inputs would be 130 to 790 MB, and their launches have n rows, not L).  Every file they
    write byte for byte against numpy."""
    import regimes_truth as R0
    from eagleeverything_amd import rcpp_api
    loader_regime(n, L)
    Mt8, planted = loader_panel(n, L)
    M8 = np.ascontiguousarray(Mt8.T)
    dims = (n, L)

    def check_files(fM, fMt, G8, who):
        Gt8 = np.ascontiguousarray(G8.T)
        assert read(fM) == R.text_of(G8).tobytes() and read(fMt) == R.text_of(Gt8).tobytes(), who
        assert read(fMt + ".e2b")[E2B_HEADER:] == R.pack2b_rows(Gt8).tobytes() and read(fM + ".e2b")[E2B_HEADER:] == R.pack2b_rows(G8).tobytes(), who
        assert np.array_equal(rcpp_api.marker_counts(fMt, dims), R.counts_of(Gt8)), who
    # ---- the .bed file
    b = tmp_path / "bed"
    b.mkdir()
    bed = R0.write_codes(str(b / "p.bed"), np.array([0, 2, 3], dtype=np.uint8)[Mt8 + 1])
    fM, fMt = str(b / "M.ascii"), str(b / "Mt.ascii")
    rcpp_api.drop_cache()
    assert rcpp_api.create_ascii_from_bed(bed, fM, fMt, 8.0, [n, L]) == 0
    check_files(fM, fMt, M8, "bed")
    # ---- filter_markers: every marker but one beside each planted one and a run in the middle
    gone = np.unique(np.concatenate((np.clip(planted + 2, 0, L - 1), np.arange(1000, 1200))))
    gone = gone[~np.isin(gone, planted)]
    keep = np.setdiff1d(np.arange(L), gone)
    assert (keep.size > R.BAND_ROWS) == (L == 196700)
    q = tmp_path / "qc"
    q.mkdir()
    assert rcpp_api.filter_markers(fM, fMt, dims, keep, str(q / "M.ascii"), str(q / "Mt.ascii")) == [n, keep.size]
    assert read(str(q / "Mt.ascii")) == R.text_of(Mt8[keep]).tobytes() and read(str(q / "M.ascii")) == R.text_of(M8[:, keep]).tobytes()
    assert read(str(q / "Mt.ascii.e2b"))[E2B_HEADER:] == R.pack2b_rows(Mt8[keep]).tobytes()
    assert np.array_equal(rcpp_api.marker_counts(str(q / "Mt.ascii"), (n, keep.size)), R.counts_of(Mt8[keep]))
    rcpp_api.drop_cache()                                                      # and cold: from the sidecars the filter wrote
    assert np.array_equal(rcpp_api.marker_counts(str(q / "Mt.ascii"), (n, keep.size)), R.counts_of(Mt8[keep]))
    rcpp_api.drop_cache()
    if n != 37:
        return
    # ---- the text table
    d = tmp_path / "text"
    d.mkdir()
    table = np.full((n, 2 * L), ord(" "), dtype=np.uint8)
    table[:, 0::2] = M8 + 1 + ord("0")
    table[:, -1] = ord("\n")
    table.tofile(str(d / "table.txt"))
    fM, fMt = str(d / "M.ascii"), str(d / "Mt.ascii")
    assert rcpp_api.createM_ASCII_rcpp(str(d / "table.txt"), fM, "text", 0, 1, 2, 8.0, dims)
    rcpp_api.createMt_ASCII_rcpp(fM, fMt, "text", 8.0, dims)
    check_files(fM, fMt, M8, "text")
    rcpp_api.drop_cache()
    # ---- the PLINK .ped file
    d = tmp_path / "plink"
    d.mkdir()
    ped, Mp8 = ped_bytes(M8)
    assert (Mp8[0] <= 0).all() and (Mp8 != M8).any()
    with open(str(d / "p.ped"), "wb") as f:
        f.write(ped)
    fM, fMt = str(d / "M.ascii"), str(d / "Mt.ascii")
    assert rcpp_api.createM_ASCII_rcpp(str(d / "p.ped"), fM, "PLINK", "-9", "-9", "-9", 8.0, [n, 6 + 2 * L])
    rcpp_api.createMt_ASCII_rcpp(fM, fMt, "PLINK", 8.0, dims)
    check_files(fM, fMt, Mp8, "PLINK")
    rcpp_api.drop_cache()


# ================================================================================================ b. the arg-max
ARGMAX_LS = [1, 255, 256, 257, 262144, 262145, 1000003]


@pytest.mark.parametrize("L", ARGMAX_LS)
def test_gpu_tsq_argmax_planted_ties_nan_and_infinities(L):
    """eagle_dev_tsq_argmax on device vectors, the way sharded.py calls it: the first index of the maximum with NaN ignored, across lanes,
    waves, blocks, the trips of the grid-stride loop and the 1,024 partials; near_ties under the kernel's own rule; tsq_out bit for bit
    (NaN for NaN)."""
    torch, lib, ctx, dev, stream = _ctx()
    blocks, trips = R.argmax_grid(L)
    assert (blocks, trips) == {1: (1, 1), 255: (1, 1), 256: (1, 1), 257: (2, 1), 262144: (1024, 1), 262145: (1024, 2), 1000003: (1024, 4)}[L]
    names = sorted(R.argmax_plants(L))
    assert ("trips" in names) == (trips >= 2) and ("blocks" in names) == (blocks >= 2)
    say(L=L, blocks=blocks, trips=trips, cases=",".join(names))
    scratch = torch.zeros(3 * 1024, dtype=torch.float64, device=dev)
    best = torch.zeros(3, dtype=torch.int64, device=dev)                       # eagle_best: {f64, i64, i64}
    for name in names:
        a, vara, want = R.argmax_case(L, name)
        tsq, idx, mx, near = R.tsq_truth(a, vara)
        assert idx == want, (L, name)
        ta, tv = torch.from_numpy(a).to(dev), torch.from_numpy(vara).to(dev)
        for with_tsq in (False, True):
            out = torch.full((L,), 7.0, dtype=torch.float64, device=dev) if with_tsq else None
            scratch.fill_(1e300)                                               # stale partials must not be read
            best.fill_(-5)
            assert lib.eagle_dev_tsq_argmax(ctx, ta.data_ptr(), tv.data_ptr(), L, out.data_ptr() if with_tsq else None, best.data_ptr(),
                                            scratch.data_ptr(), stream) == 0
            torch.cuda.synchronize()
            b = best.cpu().numpy()
            got_mx = float(b[:1].view(np.float64)[0])
            assert int(b[1]) == idx, (L, name, with_tsq, int(b[1]), idx)
            assert (np.isnan(got_mx) and idx == -1) or b[0] == np.float64(mx).view(np.int64), (L, name, got_mx, mx)
            assert int(b[2]) == near, (L, name, with_tsq, int(b[2]), near)
            if with_tsq:
                assert np.array_equal(bits(out.cpu().numpy()), bits(tsq)), (L, name)
        assert torch.equal(ta.cpu(), torch.from_numpy(a)) and torch.equal(tv.cpu(), torch.from_numpy(vara))     # only read


def test_gpu_scan_argmax_tie_between_two_trips_from_a_file(tmp_path, oracle):
    """A scan at n = 20 and L = 300,007 whose strongest marker has an exact copy 262,144 lines away: the same thread of k_tsq_partial
    meets both, in two trips, and the first must be selected -- the oracle's index."""
    from eagleeverything_amd import rcpp_api
    n, L = 20, 300007
    blocks, trips = R.argmax_grid(L)
    assert (blocks, trips) == (1024, 2)
    rng = np.random.default_rng(11)
    Mt8 = rng.integers(-1, 2, size=(L, n)).astype(np.int8)
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    S = A @ A.T + np.eye(n)
    V = 0.5 * np.eye(n) - 0.01 * np.outer(A[:, 0], A[:, 0])
    ahat = rng.standard_normal(n)
    fMt = str(tmp_path / "Mt.ascii")
    R.text_of(Mt8).tofile(fMt)
    exp = oracle.calculate_a_and_vara_rcpp(fMt, np.nan, S, V, 8.0, (L, n), ahat)
    s = oracle.tsq_argmax(exp["a"], exp["vara"])[1] - 1
    twin = s + R.ARGMAX_ONE_TRIP if s + R.ARGMAX_ONE_TRIP < L else s - R.ARGMAX_ONE_TRIP
    assert 0 <= twin < L and abs(twin - s) == 262144
    Mt8[twin] = Mt8[s]
    R.text_of(Mt8).tofile(fMt)
    a_ref, v_ref = exp["a"].copy(), exp["vara"].copy()
    a_ref[twin], v_ref[twin] = a_ref[s], v_ref[s]                             # a marker's a and vara depend on its own line alone
    _, idx_ref, mx_ref = oracle.tsq_argmax(a_ref, v_ref)
    assert idx_ref == min(s, twin) + 1
    say(n=n, L=L, blocks=blocks, trips=trips, strongest=s, twin=twin, expected_1_based=idx_ref)
    rcpp_api.drop_cache()
    res = rcpp_api.calculate_a_and_vara_rcpp(fMt, np.nan, S, V, 8.0, (L, n), ahat)
    idx, mx, ties = rcpp_api.last_scan_argmax()
    assert res["a"][s] == res["a"][twin] and res["vara"][s] == res["vara"][twin]
    _, idx_dev, mx_dev, near_dev = R.tsq_truth(res["a"], res["vara"])         # the rule on the device's own numbers
    assert idx == idx_dev + 1 and mx == mx_dev and ties == near_dev >= 2
    assert idx == idx_ref and abs(mx - mx_ref) <= 1e-6 * mx_ref
    rcpp_api.drop_cache()


# ================================================================================================ c. line scores
SCORE_LS = {262143: 1, 262144: 1, 262145: 2, 600011: 3}


@functools.lru_cache(maxsize=1)
def score_base():
    base = R.base_panel(1021, 20, seed=20)
    base.setflags(write=False)
    return base


@pytest.mark.parametrize("T", [1, 64])
@pytest.mark.parametrize("L", sorted(SCORE_LS))
def test_gpu_marker_scores_across_the_chunk_of_262144_lines(tmp_path, L, T):
    from eagleeverything_amd import r_api, rcpp_api
    from scores_truth import edge_weights, np_scores
    n, P = 20, 1021
    chunks = R.score_chunks(L)
    assert chunks == SCORE_LS[L] and (chunks >= 2) == (L > R.SCORE_CHUNK_LINES)
    base = score_base()
    planted = R.planted_markers(L, P, edges=(R.SCORE_CHUNK_LINES,))
    assert (L <= 262144 or {262143, 262144}.issubset(planted.tolist())) and planted[-1] == L - 1
    fMt = str(tmp_path / "Mt.ascii")
    rows = R.write_periodic(fMt, base, L, planted)
    v = edge_weights(T, n, seed=T)
    live = R.score_digits(v).any(axis=(1, 2))
    assert live.all()                                                          # four digit planes
    base_scores, row_scores = r_api.line_scores_host(base, v), r_api.line_scores_host(rows, v)
    assert np.array_equal(base_scores, np_scores(base, v)) and base_scores.dtype == np.int64
    assert (row_scores != base_scores[planted % P]).any(axis=1).all()          # a planted line is told from the line it replaces
    say(n=n, L=L, T=T, chunks=chunks, lines_in_last_chunk=L - (chunks - 1) * R.SCORE_CHUNK_LINES, planes=int(live.sum()), planted=planted.size)
    rcpp_api.drop_cache()
    got = rcpp_api.marker_scores(fMt, (n, L), v)
    assert got.dtype == np.int64 and got.shape == (L, T)
    assert_periodic(got, base_scores, planted, row_scores, "marker_scores")
    rcpp_api.drop_cache()


def test_gpu_sample_scores_at_the_longest_line(tmp_path):
    """n = 2 at EAGLE_SCORES_MAX_LINE with T = 64 and four live planes: 256 rows of B, rowsB * ld = 2^31 - 32,768 in k_line_scores_i8's
    int, and plane sums of 128 C in the int32 accumulators (digit -128 against g = -1 on every character)."""
    from eagleeverything_amd import _lib, rcpp_api
    n, Cn, T, P = 2, R.SCORES_MAX_LINE, 64, 4099
    assert 4 * T * Cn == 2147450880 == 2 ** 31 - 32768 and 128 * Cn == 1073725440 < 2 ** 31
    w_tile = R.capacity_score_tile(T, P, seed=9)
    assert R.score_digits(w_tile).any(axis=(1, 2)).all() and R.score_digits(w_tile[0])[:3].min() == -128
    g_tile = np.stack([np.full(P, -1, dtype=np.int8), R.base_panel(P, 1, seed=3)[:, 0]])
    reps = -(-Cn // P)
    g = np.tile(g_tile, (1, reps))[:, :Cn]
    w = np.ascontiguousarray(np.tile(w_tile, (1, reps))[:, :Cn])
    want = R.tiled_scores(w_tile, g_tile, Cn)
    assert want[0, 0] == -R.SCORE_FULL_DIGITS * Cn and want[0, 1] == R.SCORES_MAX_WEIGHT * Cn
    for c in (0, Cn // 2, Cn - 1):                                             # off the period: -2^30 against g = -1 at both ends and the middle
        new_g, new_w = g[:, c].copy(), w[:, c].copy()
        new_g[1], new_w[3] = -1, -R.SCORES_MAX_WEIGHT
        want += np.outer(new_g.astype(np.int64), new_w.astype(np.int64)) - np.outer(g[:, c].astype(np.int64), w[:, c].astype(np.int64))
        g[:, c], w[:, c] = new_g, new_w
    fM = str(tmp_path / "M.ascii")
    R.text_of(g).tofile(fM)
    say(n=n, C=Cn, T=T, planes=4, rowsB=4 * T, rowsB_times_ld=4 * T * Cn, largest_plane_sum=128 * Cn, stages=Cn // 128)
    lib, ctx = _lib.load(), rcpp_api.context(0)
    out = np.zeros((n, T), dtype=np.int64)
    rcpp_api.drop_cache()
    rcpp_api._check(ctx, lib.eagle_sample_scores(ctx, os.fsencode(fM), rcpp_api._dims((n, Cn)), w.ctypes.data_as(C.POINTER(C.c_int32)), T, 8.0,
                                                 out.ctypes.data_as(C.POINTER(C.c_int64))))
    assert np.array_equal(out, want), np.argwhere(out != want)[:5].tolist()
    rcpp_api.drop_cache()


# ================================================================================================ d. weighted_gram at its capacity
def test_gpu_weighted_gram_at_the_marker_capacity(tmp_path, monkeypatch):
    """n = 2 at EAGLE_WGRAM_MAX_MARKERS with every digit of every weight 127: the three plane accumulators reach 127 L = 2^31 - 8 on the
    diagonal and climb to 127 L / 2 before they return to 0 off it.  Resident, then in nine marker windows: the accumulators are not
    folded between windows."""
    from eagleeverything_amd import rcpp_api
    n, L, q = 2, R.WGRAM_MAX_MARKERS, R.WGRAM_MAX_WEIGHT
    assert 127 * L == 2 ** 31 - 8 and q == 127 + 127 * 128 + 127 * 128 * 128 and L % 2 == 0
    g = np.ones((n, L), dtype=np.int8)
    g[1, L // 2:] = -1
    fM = str(tmp_path / "M.ascii")
    R.text_of(g).tofile(fM)
    qv = np.full(L, q, dtype=np.uint32)
    want = R.wgram_capacity_truth(L, q)
    assert want.tolist() == [[q * L, 0], [0, q * L]]
    rcpp_api.drop_cache()
    got = rcpp_api.weighted_gram(fM, (n, L), qv)
    assert got.dtype == np.int64 and np.array_equal(got, want), got.tolist()
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "1")
    Lw = R.stream_window(10 ** 9, 256, R.pad(L))
    windows = -(-L // Lw)
    assert (Lw, windows) == (1953024, 9)
    got = rcpp_api.weighted_gram(fM, (n, L), qv)
    st = rcpp_api.last_stream_stats()
    assert st["chunks"] == windows, st
    assert np.array_equal(got, want), got.tolist()
    say(n=n, L=L, q=q, plane_sum=127 * L, off_diagonal_peak=127 * (L // 2), window_markers=Lw, windows=windows)
    monkeypatch.delenv("EAGLE_HIP_MAX_RESIDENT_GB")
    rcpp_api.drop_cache()


# ================================================================================================ e. offsets past 2^32
BIG_N, BIG_L, BIG_P = 7, 16777300, 4099
BIG_LD = 256


@pytest.fixture(scope="module")
def big_panel(tmp_path_factory):
    """(Mt.ascii, M.ascii or None, base, planted markers, planted lines): 7 individuals and 16,777,300 markers, 134 MB of text and a
    resident image of 4.3 GB whose rows lie past 2^31 bytes from marker 8,388,608 on and past 2^32 from 16,777,216 on; planted lines on
    both sides of both.  The files are deleted when the module is done."""
    from eagleeverything_amd import rcpp_api
    d = tmp_path_factory.mktemp("big")
    base = R.base_panel(BIG_P, BIG_N, seed=7)
    planted = R.planted_markers(BIG_L, BIG_P, edges=(2 ** 31 // BIG_LD,))
    assert {2 ** 31 // 256 - 1, 2 ** 31 // 256, 2 ** 32 // 256 - 1, 2 ** 32 // 256, 2 ** 32 // 256 + 1, BIG_L - 1}.issubset(planted.tolist())
    assert R.pad(BIG_N) == BIG_LD and (BIG_L - 1) * BIG_LD > 2 ** 32 and R.pad(BIG_L) * BIG_LD == 4295032832
    fMt = str(d / "Mt.ascii")
    rows = R.write_periodic(fMt, base, BIG_L, planted)
    assert os.path.getsize(fMt) == BIG_L * (BIG_N + 1) < 150e6
    for a in (base, planted, rows):
        a.setflags(write=False)
    rcpp_api.drop_cache()
    yield fMt, base, planted, rows
    rcpp_api.drop_cache()
    os.remove(fMt)


def big_regime(**more):
    say(n=BIG_N, L=BIG_L, ld=BIG_LD, image_bytes=R.pad(BIG_L) * BIG_LD, first_row_past_2_31=2 ** 31 // BIG_LD, first_row_past_2_32=2 ** 32 // BIG_LD, **more)


def test_gpu_big_panel_marker_counts(big_panel):
    from eagleeverything_amd import rcpp_api
    fMt, base, planted, rows = big_panel
    big_regime(out_bytes=BIG_L * 12)
    got = rcpp_api.marker_counts(fMt, (BIG_N, BIG_L))
    assert (got.sum(axis=1) == BIG_N).all()
    assert_periodic(got, R.counts_of(base), planted, R.counts_of(rows), "marker_counts")


@pytest.mark.parametrize("K", [2, 33])
def test_gpu_big_panel_group_counts(big_panel, K):
    from eagleeverything_amd import r_api, rcpp_api
    fMt, base, planted, rows = big_panel
    labels = np.array([0, 1, 0, 1, -1, 1, 0]) if K == 2 else np.array([0, 32, 5, 32, -1, 17, 0])
    big_regime(K=K, out_bytes=BIG_L * K * 12, out_past_2_32=BIG_L * K * 12 > 2 ** 32)
    assert (BIG_L * K * 12 > 2 ** 32) == (K == 33)
    got = rcpp_api.group_counts(fMt, (BIG_N, BIG_L), labels, K)
    assert got.shape == (BIG_L, K, 3)
    base_counts = r_api.group_counts_host(base, labels, K)
    assert np.array_equal(base_counts.sum(axis=1), R.counts_of(base[:, labels >= 0]))
    assert_periodic(got, base_counts, planted, r_api.group_counts_host(rows, labels, K), "group_counts")


def test_gpu_big_panel_marker_scores(big_panel):
    from eagleeverything_amd import r_api, rcpp_api
    from scores_truth import edge_weights
    fMt, base, planted, rows = big_panel
    v = edge_weights(2, BIG_N, seed=5)
    chunks = R.score_chunks(BIG_L)
    assert chunks == 65
    big_regime(T=2, score_chunks=chunks)
    got = rcpp_api.marker_scores(fMt, (BIG_N, BIG_L), v)
    assert_periodic(got, r_api.line_scores_host(base, v), planted, r_api.line_scores_host(rows, v), "marker_scores")


def test_gpu_big_panel_logistic(big_panel, tmp_path):
    """Intercept and one covariate.  The large panel against the same call on the base panel's own file, bit for bit; on the base
    panel, which markers cannot be fitted (monomorphic among the used individuals) and the score of the others against
    r_api.logistic_host, which is not bit-equal to the device (tests/test_gpu_logistic.py holds both to 40-digit roots)."""
    from eagleeverything_amd import r_api, rcpp_api
    fMt, base, planted, rows = big_panel
    status = np.array([1, 0, 1, 0, 1, 0, -1])
    X = np.stack([np.ones(BIG_N), np.array([0.3, -1.2, 0.7, 0.1, -0.4, 1.5, 0.0])], axis=1)
    small = np.concatenate((base, rows))
    fs = str(tmp_path / "small.ascii")
    R.text_of(small).tofile(fs)
    s_stat, s_info = rcpp_api.logistic(fs, (BIG_N, small.shape[0]), status, X)
    used = status >= 0
    mono = (small[:, used] == small[:, used][:, :1]).all(axis=1)               # no fit: the score is NaN and the code 2 after one evaluation
    assert mono[:3].all() and 0.05 < mono.mean() < 0.9
    assert np.array_equal(np.isnan(s_stat[:, 2]), mono) and (s_info[mono, 0] == 2).all() and (s_info[mono, 1] == 1).all()
    some = np.concatenate((np.arange(200), np.arange(BIG_P, small.shape[0])))  # the restatement is a Python loop over the markers
    h_stat, h_info = r_api.logistic_host(small[some], status, X)
    assert np.array_equal(np.isnan(h_stat[:, 2]), mono[some]) and (h_info[mono[some], 0] == 2).all()
    fin = ~mono[some]
    assert np.allclose(s_stat[some][fin, 2], h_stat[fin, 2], rtol=1e-9, atol=1e-12)       # the score: two fp64 evaluations of the same sums
    big_regime(out_bytes=BIG_L * 32)
    stat, info = rcpp_api.logistic(fMt, (BIG_N, BIG_L), status, X)
    assert_periodic(info, s_info[:BIG_P], planted, s_info[BIG_P:], "logistic info")
    assert_periodic(bits(stat), bits(s_stat[:BIG_P]), planted, bits(s_stat[BIG_P:]), "logistic stat")


def seam_slices(L, planted, reach):
    """[(lo, hi)]: the runs of markers within `reach` of a planted line or of either end of the file, where a cross-line result is not the
    periodic interior's."""
    special = set(range(min(reach, L))) | set(range(max(0, L - reach), L))
    for p in np.asarray(planted).tolist():
        special.update(range(max(0, p - reach), min(L, p + reach + 1)))
    s = sorted(special)
    runs, lo = [], s[0]
    for a, b in zip(s, s[1:] + [None]):
        if b != a + 1:
            runs.append((lo, a))
            lo = b
    return runs


def panel_slice(base, planted, a, b):
    pl = set(np.asarray(planted).tolist())
    return np.stack([R.planted_line(m, base.shape[1]) if m in pl else base[m % base.shape[0]] for m in range(a, b)])


def cross_line_check(got, L, base, planted, reach, host, what):
    """got: a per-marker result in marker-relative form.  host(lines) -> the same from a block of consecutive lines taken as a whole
    file.  Interior: the middle period of three; seams: host on the lines around them, `reach` more on either side."""
    P = base.shape[0]
    interior = host(np.tile(base, (3, 1)))[P:2 * P]
    seams = seam_slices(L, planted, reach)
    ms, wants = [], []
    for lo, hi in seams:
        a, b = max(0, lo - reach), min(L, hi + 1 + reach)
        r = host(panel_slice(base, planted, a, b))
        ms.extend(range(lo, hi + 1))
        wants.extend(r[lo - a:hi + 1 - a])
    assert_periodic(got, interior, np.array(ms), wants, what)
    return len(seams)


def test_gpu_big_panel_ld(big_panel):
    """Window 3: ld_partners (partners as offsets from their marker, r2 bits) and ld_stats, restated at the seams -- both ends of the file
    and around every planted line -- and in the periodic interior from three periods of the base panel; ld_dots at three loci."""
    from eagleeverything_amd import r_api, rcpp_api
    fMt, base, planted, rows = big_panel
    w, l, dims = 3, 4, (BIG_N, BIG_L)
    big_regime(window=w, l=l, band_bytes=BIG_L * w * 8)
    NONE = np.int32(-(2 ** 30))

    def partners_rel(lines, first=0):
        p, r2 = r_api.ld_partners_host(lines, w, l, 0.0)
        m = np.arange(lines.shape[0], dtype=np.int32)[:, None]
        return np.where(p >= 0, p - m, NONE).astype(np.int32), bits(r2)
    part, r2 = rcpp_api.ld_partners(fMt, dims, window=w, l=l, return_r2=True)
    rel = np.where(part >= 0, part - np.arange(BIG_L, dtype=np.int32)[:, None], NONE).astype(np.int32)
    seams = cross_line_check(rel, BIG_L, base, planted, w, lambda g: partners_rel(g)[0], "ld_partners")
    cross_line_check(bits(r2), BIG_L, base, planted, w, lambda g: partners_rel(g)[1], "ld_partners r2")

    def stats(lines):
        U, cnt = r_api.ld_stats_host(r_api.ld_band_host(lines, w))[:2]
        return np.stack([U.astype(np.int64), cnt.astype(np.int64)], axis=1)
    U, cnt = rcpp_api.ld_stats(fMt, dims, window=w)
    assert U.dtype == np.uint64 and cnt.dtype == np.int32
    cross_line_check(np.stack([U.astype(np.int64), cnt.astype(np.int64)], axis=1), BIG_L, base, planted, w, stats, "ld_stats")
    loci = np.array([5, 2 ** 31 // 256 + 1, BIG_L - 40])
    assert BIG_L - 100 <= loci[2] < BIG_L
    dots = rcpp_api.ld_dots(fMt, dims, loci)
    cols = np.stack([panel_slice(base, planted, int(j), int(j) + 1)[0] for j in loci]).astype(np.int64)       # (3, n)
    assert dots.dtype == np.int32 and dots.shape == (BIG_L, 3)
    assert_periodic(dots, (base.astype(np.int64) @ cols.T).astype(np.int32), planted, (rows.astype(np.int64) @ cols.T).astype(np.int32), "ld_dots")
    say(seams=seams)


# ---- the device kernels called directly, at the large panel's image size and at their band edges
def periodic_image(torch, dev, rows, ld, P=BIG_P):
    """int8 (rows, ld) on the device: P random lines of {-1, 0, +1} repeated, lines 1, rows - 2 all -1 and all +1."""
    g = np.random.default_rng(rows).integers(-1, 2, size=(P, ld)).astype(np.int8)
    img = torch.from_numpy(g).to(dev).repeat(-(-rows // P), 1)[:rows].contiguous()
    img[1], img[rows - 2] = -1, 1
    return img, g


def test_gpu_pack_2bit_round_trip_at_the_big_image():
    """k_pack_2bit: 65,536 blocks of 256 threads make 17 trips over the 268 million sixteen-byte pieces of a 4.3 GB image."""
    torch, lib, ctx, dev, stream = _ctx()
    L_pad, ld = R.pad(BIG_L), BIG_LD
    blocks, trips = R.pack2_grid(L_pad, ld)
    assert (blocks, trips) == (65536, 17) and L_pad * ld > 2 ** 32
    say(L_pad=L_pad, ld=ld, pieces=L_pad * ld // 16, blocks=blocks, trips=trips, rows_per_trip=R.PACK2_ONE_TRIP // 16)
    img, g = periodic_image(torch, dev, L_pad, ld)
    Mt2 = torch.full((L_pad, ld // 4), 0xA5, dtype=torch.uint8, device=dev)
    assert lib.eagle_dev_pack_2bit(ctx, img.data_ptr(), L_pad, ld, ld, Mt2.data_ptr(), stream) == 0
    back = torch.full_like(img, 7)
    assert lib.eagle_dev_unpack_2bit(ctx, Mt2.data_ptr(), L_pad, ld, ld, back.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(back, img)
    # the layout rule of tests/test_gpu_gemv_2bit.py on the rows around every trip edge, the first and the last
    per = R.PACK2_ONE_TRIP // (ld // 16)
    sample = sorted({0, 1, L_pad - 2, L_pad - 1} | {r + o for r in range(per, L_pad, per) for o in (-1, 0, 1)})
    k = np.arange(ld)
    word, bit = 16 * (k >> 8) + 4 * ((k >> 4) & 3) + ((k >> 6) & 3), 8 * (k & 3) + 2 * ((k >> 2) & 3)
    idx = torch.tensor(sample, device=dev)
    words = Mt2[idx].cpu().numpy().view(np.uint32)
    lines = img[idx].cpu().numpy()
    assert np.array_equal((words[:, word] >> bit.astype(np.uint32)) & 3, lines.astype(np.uint8) & 3)
    want = g[np.array(sample) % BIG_P]
    want[sample.index(1)], want[sample.index(L_pad - 2)] = -1, 1
    assert np.array_equal(lines, want)                                         # the image was only read


@pytest.mark.parametrize("count", [2 ** 22 + 4, 2 ** 29 + 4])
def test_gpu_add_i32_past_one_trip_of_its_grid(count):
    torch, lib, ctx, dev, stream = _ctx()
    trips = R.add_trips(count)
    assert trips == {2 ** 22 + 4: 3, 2 ** 29 + 4: 257}[count] and (count // 4) % (R.ADD_GRID * 256) == 1
    say(count=count, bytes=4 * count, grid=R.ADD_GRID, trips=trips, elements_in_last_trip=4)
    fn = lib.eagle_dev_add_i32
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    i = torch.arange(count, dtype=torch.int64, device=dev)
    dst = (i % 1000003).to(torch.int32)
    src = ((i * 7) % 999983 - 400000).to(torch.int32)
    del i
    dst[-1], src[-1] = 2 ** 31 - 1, 1                                          # wraps like int32
    want = dst + src
    src0 = src.clone()
    assert fn(ctx, dst.data_ptr(), src.data_ptr(), count, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, want) and torch.equal(src, src0)
    at = [0, 1, R.ADD_ONE_TRIP - 1, R.ADD_ONE_TRIP, count - 5, count - 2]
    assert dst[at].tolist() == [(j % 1000003) + ((j * 7) % 999983 - 400000) for j in at] and int(dst[-1]) == -2 ** 31


def test_gpu_transpose_i8_second_band_of_64_x_65535_rows():
    torch, lib, ctx, dev, stream = _ctx()
    rows, cols = R.TRANSPOSE_BAND_ROWS + 128, 64
    bands = R.bands(rows, R.TRANSPOSE_BAND_ROWS)
    assert bands == [(0, 4194240), (4194240, 128)]
    say(rows=rows, cols=cols, bands=len(bands), rows_in_second_band=bands[1][1])
    src, _ = periodic_image(torch, dev, rows, cols)
    out = torch.full((cols, rows), 7, dtype=torch.int8, device=dev)
    assert lib.eagle_dev_transpose_i8(ctx, src.data_ptr(), rows, cols, cols, out.data_ptr(), rows, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, src.t().contiguous())
    assert out[:, 1].eq(-1).all() and out[:, rows - 2].eq(1).all()


@pytest.mark.parametrize("L_pad", [65535, 65536, 65537, 196864])
def test_gpu_pack_fp4_bands_over_the_markers(L_pad):
    torch, lib, ctx, dev, stream = _ctx()
    ld = 256
    bands = R.bands(L_pad)
    assert len(bands) == {65535: 1, 65536: 2, 65537: 2, 196864: 4}[L_pad]
    say(L_pad=L_pad, ld=ld, bands=len(bands), rows_in_last_band=bands[-1][1])
    img, g = periodic_image(torch, dev, L_pad, ld, P=1021)
    out = torch.full((L_pad, ld // 2), 0x55, dtype=torch.uint8, device=dev)
    assert lib.eagle_dev_pack_fp4(ctx, img.data_ptr(), L_pad, ld, ld, out.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    want = R.fp4_rows(img.cpu().numpy())
    got = out.cpu().numpy()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, bad[:5].tolist()
    assert (got[1] == 0xAA).all() and (got[L_pad - 2] == 0x22).all()
