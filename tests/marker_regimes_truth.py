"""Restated launch arithmetic and builders for tests/test_gpu_marker_regimes.py: every number that makes a path of the library depend
on the marker count L, on the number of lines of a file or on an image's byte size, as plain arithmetic, and the periodic panels whose
truth at millions of markers costs one small base panel.  CPU only; tests/test_marker_regimes_host.py pins every constant to the
source text and every builder to plain loops.

Survey of csrc/: the branches that switch on L, on rows per window or on an image's byte size, and where each one runs in the suite
("here" = tests/test_gpu_marker_regimes.py).

  covered here
    eagle_dev_decode_ascii, eagle_dev_encode_ascii, eagle_dev_pack2b, eagle_dev_unpack2b (eagle_kernels.hip): row bands of 65,535
        (gridDim.y), both pointers advanced by r0 * stride -- family a, through the files; a staged chunk holds 67,108,864 / stride rows
        (stream_rows and scan_lines of eagle_load.cpp, create_M_text / eagle_create_Mt_ascii / SidecarWriter of eagle_ingest.cpp)
    eagle_dev_decode_ascii_cols, eagle_dev_unpack2b_cols, eagle_dev_gather_cols_i8: the same row counts through a VIEW alias -- family a
    eagle_dev_pack_fp4 (eagle_i8mfma.hip): bands of 65,535 over L_pad -- direct call, family e
    eagle_dev_transpose_i8: bands of 64 x 65,535 rows -- direct call, family e (no entry point hands it more than pad256(n) rows
        below n = 4,194,240 individuals)
    eagle_dev_tsq_argmax: grid capped at 1,024 blocks of 256, second trip of k_tsq_partial / k_tsq_near from L = 262,145 -- family b
    eagle_dev_line_scores (eagle_score.hip): chunks of SCORE_CHUNK_TILES = 1,024 row tiles = 262,144 lines -- family c
    k_line_scores_i8: rowsB * ld in int at ld = EAGLE_SCORES_MAX_LINE, four planes, T = 64 -- family c, sample_scores at the capacity
    eagle_wgram (eagle_api.cpp): the int32 plane accumulators at 127 L = 2^31 - 8, resident and across marker windows -- family d
    k_pack_2bit: grid capped at 65,536 blocks, second trip above 16,777,216 sixteen-byte pieces -- direct call, family e
    k_add_i32: fixed grid of 2,048 blocks, second trip above 2,097,152 elements -- direct call, family e
    row * ld, counts[row * 3 + lane], band[gi * window + o] past 2^31 and 2^32 bytes (eagle_qc.hip, eagle_groups.hip, eagle_logit.hip,
        eagle_ld.hip, eagle_score.hip) -- family e, n = 7 and L = 16,777,300
  covered elsewhere
    eagle_dev_plane_gather (65,535 words a launch), parentage_chunk (65,535 offspring): tests/test_gpu_regimes.py
        test_gpu_plane_gather_second_batch_of_words, test_gpu_parentage_second_chunk_of_offspring
    stream_chunk_rows_core (256-marker windows under EAGLE_HIP_MAX_RESIDENT_GB): tests/test_gpu_marker_qc.py
        test_gpu_marker_counts_resident_streamed_sidecar, tests/test_gpu_scores.py test_gpu_scores_streamed_equals_resident
    bed_window_markers / the .bed staging ring: tests/test_gpu_bed.py, tests/test_gpu_regimes.py (rows of 256 to 16,385 bytes)
    vara_piped (n_pad >= 65,536), EXT_CAP_MAX = 65,536 re-evaluated markers: tests/test_gpu_scan_exact.py, tests/test_gpu_lastdigit_exact.py
    k_tiles_pack (65,536 int32 a tile), n_pad / 256 <= 65,535: tests/test_multi_device.py
  out of reach
    eagle_dev_decode_ascii's refusal at rows > 65,535 x 32,768 = 2^31 - 32,768 lines: one staged chunk never holds more than 67,108,864
    L > 0x7fffffff (eagle_dev_plane_gather, eagle_parentage, eagle_weighted_gram, the scores' "more than 2^31 - 1 lines"): a 2 GiB
        file per individual; the refusals are pinned by the test_*_abi.py
    eagle_dev_transpose_i8's second band from an entry point: needs pad256(n) > 4,194,240 individuals
    L_pad / 256 > 65,535 (eagle_bedibs.hip) and nblocks >= 2^30 (eagle_grm.hip, eagle_score.hip): L >= 16,776,960 markers in ONE
        window of a sample-major fp4 image / more than 2^30 workgroups, i.e. n >= 4 million lines of 8 million characters
    ld * 256 >= 2^31 for a resident 256-padded image (line_scores' `narrow`): reached here only on its narrow side (family c)
"""
import numpy as np

# csrc/eagle_load.cpp, csrc/eagle_ingest.cpp: bytes of one staging buffer
STAGE_BYTES = 67108864
# csrc/eagle_kernels.hip, csrc/eagle_i8mfma.hip: rows of one launch whose gridDim.y is the row
BAND_ROWS = 65535
TRANSPOSE_BAND_ROWS = 64 * 65535
# eagle_dev_tsq_argmax
ARGMAX_BLOCKS = 1024
ARGMAX_THREADS = 256
ARGMAX_ONE_TRIP = ARGMAX_BLOCKS * ARGMAX_THREADS          # 262,144
# csrc/eagle_score.hip, csrc/eagle_t8.h
SCORE_CHUNK_TILES = 1024
T8 = 256
SCORE_CHUNK_LINES = SCORE_CHUNK_TILES * T8                # 262,144
# k_pack_2bit, k_add_i32
PACK2_GRID_CAP = 65536
PACK2_ONE_TRIP = PACK2_GRID_CAP * 256                     # 16,777,216 sixteen-byte pieces
ADD_GRID = 2048
ADD_ONE_TRIP = ADD_GRID * 256 * 4                         # 2,097,152 int32
# include/eagle_hip.h
WGRAM_MAX_MARKERS = 16909320
WGRAM_MAX_WEIGHT = (1 << 21) - 1
SCORES_MAX_LINE = 8388480
SCORES_MAX_WEIGHT = 1 << 30

PERIODS = (1021, 4099)


def pad(x, m=256):
    return (x + m - 1) // m * m


def text_rows_per_chunk(n):
    """Lines of n characters and a line end in one staging buffer (stream_rows' cap_bytes / stride, create_M_text's chunk_rows)."""
    return max(1, STAGE_BYTES // (n + 1))


def sidecar_rows_per_chunk(n):
    """Rows of the 2-bit sidecar in one staging buffer: ceil(n / 4) bytes staged at the next multiple of 16."""
    return max(1, STAGE_BYTES // sidecar_row_bytes(n))


def mt_window_lines(n):
    """eagle_create_Mt_ascii's marker window: the lines of n + 1 bytes that fit one staging buffer, a multiple of 256 (256 at least)."""
    return max(256, STAGE_BYTES // (n + 1) // 256 * 256)


def bands(rows, band=BAND_ROWS):
    """[(r0, nr)] of `for (r0 = 0; r0 < rows; r0 += band)`."""
    return [(r0, min(band, rows - r0)) for r0 in range(0, rows, band)]


def chunk_bands(rows, per_chunk, band=BAND_ROWS):
    """The launches of a file of `rows` rows read in chunks of per_chunk: [(first row, rows)] of every band of every chunk."""
    return [(c0 + r0, nr) for c0 in range(0, rows, per_chunk) for r0, nr in bands(min(per_chunk, rows - c0), band)]


def argmax_grid(L):
    """(blocks, trips of thread 0) of k_tsq_partial and k_tsq_near."""
    blocks = max(1, min(ARGMAX_BLOCKS, (L + 255) // 256))
    return blocks, max(1, -(-L // (blocks * ARGMAX_THREADS)))


def score_chunks(lines):
    return -(-(-(-lines // T8)) // SCORE_CHUNK_TILES)


def pack2_grid(L_pad, ld):
    """(blocks, trips of thread 0) of k_pack_2bit: one thread per 16 bytes of the int8 image."""
    total = L_pad * (ld >> 4)
    blocks = min(PACK2_GRID_CAP, (total + 255) // 256)
    return blocks, -(-total // (blocks * 256))


def add_trips(count):
    return -(-(count // 4) // (ADD_GRID * 256))


def stream_window(budget_bytes, row_bytes, total_pad):
    """stream_chunk_rows_core of csrc/eagle_host.h."""
    rows = budget_bytes // 2 // row_bytes // 256 * 256
    return min(max(rows, 256), total_pad)


# ------------------------------------------------------------------------------------------------ periodic panels
def base_panel(P, n, seed):
    """int8 (P, n) in {-1, 0, +1}: the P lines a periodic panel repeats.  Line 0 is all -1, line 1 all 0, line 2 all +1; the others are
    random with a minor allele frequency that varies by line."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.5, size=(P, 1))
    u = rng.random((P, n))
    g = (u < f * f).astype(np.int8) - (u > 1 - (1 - f) * (1 - f)).astype(np.int8)
    g[0], g[1], g[2] = -1, 0, 1
    return g


def planted_line(m, n):
    """int8 (n): the line planted at marker m -- the base-3 digits of m, least significant first, repeated along the line, minus 1.
    Lines m and m + 1 differ in their first genotype, lines less than 3^19 apart somewhere in their first 19."""
    k = min(n, 19)
    d = np.array([(m // 3 ** j) % 3 for j in range(k)], dtype=np.int8)
    return np.resize(d, n) - 1


def planted_markers(L, P, edges=(BAND_ROWS,)):
    """Where a periodic panel of L lines carries planted lines: one in the first band (marker 3), edge - 1, edge, edge + 1 around every
    multiple of every edge below L, and the last line.  Sorted, unique, inside [0, L)."""
    at = {3, L - 1}
    for e in edges:
        for k in range(e, L + 1, e):
            at.update((k - 1, k, k + 1))
    return np.array(sorted(m for m in at if 0 <= m < L), dtype=np.int64)


def periodic_lines(base, L, planted=()):
    """int8 (L, n): base repeated along the marker axis, the lines `planted` replaced by planted_line."""
    P, n = base.shape
    g = np.tile(base, (-(-L // P), 1))[:L]
    for m in np.asarray(planted, dtype=np.int64).tolist():
        g[m] = planted_line(m, n)
    return g


def text_of(g):
    """uint8 (rows, cols + 1): the fixed-width text of int8 rows, '0' '1' '2' and a line end."""
    g = np.asarray(g, dtype=np.int8)
    t = np.empty((g.shape[0], g.shape[1] + 1), dtype=np.uint8)
    t[:, :-1] = g.view(np.uint8) + np.uint8(ord("1"))
    t[:, -1] = ord("\n")
    return t


def write_periodic(path, base, L, planted=()):
    """The Mt file of periodic_lines(base, L, planted) at `path`, by one tile of the base panel's text; returns the planted lines as
    int8 (len(planted), n)."""
    P, n = base.shape
    t = np.tile(text_of(base), (-(-L // P), 1))[:L]
    planted = np.asarray(planted, dtype=np.int64)
    rows = np.stack([planted_line(m, n) for m in planted.tolist()]) if planted.size else np.zeros((0, n), dtype=np.int8)
    if planted.size:
        t[planted] = text_of(rows)
    t.tofile(path)
    return rows


def expand(base_result, L, planted, planted_result):
    """The per-marker result of a periodic panel: base_result[m mod P] with the planted markers' rows put in."""
    P = base_result.shape[0]
    out = np.tile(base_result, (-(-L // P),) + (1,) * (base_result.ndim - 1))[:L].copy()
    if len(planted):
        out[np.asarray(planted, dtype=np.int64)] = planted_result
    return out


def sidecar_row_bytes(cols):
    """sidecar_row_bytes of csrc/eagle_host.h: ceil(cols / 4) bytes at the next multiple of 16."""
    return pad((cols + 3) // 4, 16)


def pack2b_rows(g):
    """uint8 (rows, sidecar_row_bytes(cols)): the payload rows of the 2-bit sidecar, code g + 1 of column c at bits 2 (c % 4) of byte
    c / 4, zero behind the last column."""
    g = np.asarray(g, dtype=np.int8)
    rows, cols = g.shape
    c = np.zeros((rows, 4 * sidecar_row_bytes(cols)), dtype=np.uint8)
    c[:, :cols] = (g + 1).astype(np.uint8)
    c = c.reshape(rows, -1, 4)
    return (c[:, :, 0] | c[:, :, 1] << 2 | c[:, :, 2] << 4 | c[:, :, 3] << 6).astype(np.uint8)


def fp4_rows(g):
    """uint8 (rows, cols / 2): eagle_dev_pack_fp4's image, the e2m1 codes 0xA, 0x0, 0x2 of -1, 0, +1, genotype 2 k in the low nibble of
    byte k."""
    code = np.array([0xA, 0x0, 0x2], dtype=np.uint8)[np.asarray(g, dtype=np.int8) + 1]
    return (code[:, 0::2] | code[:, 1::2] << 4).astype(np.uint8)


def counts_of(g):
    """int32 (rows, 3): the numbers of -1, 0, +1 of every row."""
    g = np.asarray(g)
    return np.stack([(g == v).sum(axis=1) for v in (-1, 0, 1)], axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the arg-max
def tsq_truth(a, vara):
    """(tsq, index, tsqmax, near_ties) under k_tsq_partial / k_tsq_final / k_tsq_near's rule: tsq = a a / vara in fp64; the FIRST index of
    the largest tsq that is not NaN, -1 (and a NaN maximum) when every tsq is NaN; near_ties = the number of tsq that are not NaN and
    >= max - |max| 1e-9 (>= max when it is infinite), 0 without a maximum."""
    a, vara = np.asarray(a, dtype=np.float64), np.asarray(vara, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = (a * a) / vara
    ok = ~np.isnan(t)
    if not ok.any():
        return t, -1, float("nan"), 0
    mx = t[ok].max()
    idx = int(np.flatnonzero(ok & (t == mx))[0])
    thr = mx if np.isinf(mx) else mx - abs(mx) * 1e-9
    return t, idx, float(mx), int((ok & (t >= thr)).sum())


ARGMAX_PEAK = (10.0, 1.0)                 # a, vara of a planted maximum: tsq = 100


def argmax_background(L, seed):
    """(a, vara) fp64 (L): tsq between 0 and 4 everywhere, no NaN, no infinity."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, L), rng.uniform(1.0, 2.0, L)


def argmax_plants(L):
    """{name: (indices that get the peak, indices whose a = vara = 0 (NaN), indices whose vara = 0 alone (+inf))} for a vector of L
    entries, every case that fits L: the maximum in the last element; exact ties between two lanes of a wave, two waves of a block, two
    blocks, the two trips of one thread (i and i + 262,144); NaN at the ends and beside the maximum; +inf twice; nothing but NaN."""
    c = {"last": ([L - 1], [], []), "all_nan": ([], None, [])}
    if L >= 2:
        c["nan_ends"] = ([L // 2], sorted({0, L - 1} - {L // 2}), [])
        c["inf_twice"] = ([0], [], sorted({L // 3, L - 1}))
    if L >= 64:
        c["lanes"] = ([40, 7], [6, 8], [])
    if L >= 256:
        c["waves"] = ([200, 70], [69], [])
    if L >= 257:
        c["blocks"] = (sorted({L - 1, 255, 256}, reverse=True), [], [])
    if L > ARGMAX_ONE_TRIP:
        c["trips"] = ([L - 1, L - 1 - ARGMAX_ONE_TRIP], [5], [])
        c["trip_and_block"] = ([ARGMAX_ONE_TRIP, 3000], [], [])
    return c


def argmax_case(L, name, seed=0):
    """(a, vara, the index the case is built to select)."""
    a, vara = argmax_background(L, seed + L)
    peak, nan, inf = argmax_plants(L)[name]
    if nan is None:                       # all NaN at a large L
        a[:], vara[:] = 0.0, 0.0
        return a, vara, -1
    a[peak], vara[peak] = ARGMAX_PEAK
    if len(peak):                         # near-tie values: one inside the 1e-9 band, one outside it, both far from its edge
        free = [i for i in (1, 2) if i < L and i not in peak and i not in nan and i not in inf]
        for i, rel in zip(free, (0.25e-9, 4e-9)):
            a[i], vara[i] = 10.0, 1.0 / (1.0 - rel)
    a[nan], vara[nan] = 0.0, 0.0
    vara[inf] = 0.0
    a[inf] = 3.0
    want = min(inf) if inf else (min(peak) if peak else -1)
    return a, vara, want


# ------------------------------------------------------------------------------------------------ capacities
SCORE_FULL_DIGITS = -128 - 128 * 256 - 128 * 65536 - 63 * 16777216      # digits (-128, -128, -128, -63): three plane sums of 128 C against g = -1


def score_digits(w):
    """int64 (4, ...): the balanced base-256 digits of include/eagle_hip.h section 1b''''i."""
    w = np.asarray(w, dtype=np.int64)
    out = []
    for _ in range(4):
        d = ((w + 128) & 255) - 128
        out.append(d)
        w = (w - d) >> 8
    assert not w.any()
    return np.stack(out)


def capacity_score_tile(T, P, seed):
    """int32 (T, P): the weight tile of the sample_scores capacity case.  Column 0 is SCORE_FULL_DIGITS everywhere, column 1 is -2^30,
    column 2 is +2^30, the others random in +-2^30 with all four digit planes live."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-SCORES_MAX_WEIGHT, SCORES_MAX_WEIGHT + 1, size=(T, P)).astype(np.int32)
    w[0] = SCORE_FULL_DIGITS
    if T > 1:
        w[1] = -SCORES_MAX_WEIGHT
    if T > 2:
        w[2] = SCORES_MAX_WEIGHT
    return w


def tiled_scores(w_tile, g_tile, C):
    """int64 (rows of g_tile, T): sum_c w[t, c mod P] g[r, c mod P] over c < C, from the tile's own products: C // P whole periods and
    the first C % P columns of one more."""
    P = w_tile.shape[1]
    w, g = w_tile.astype(np.int64), np.asarray(g_tile).astype(np.int64)
    return (C // P) * (g @ w.T) + g[:, :C % P] @ w[:, :C % P].T


def wgram_capacity_truth(L, q):
    """int64 (2, 2): Q of the two individuals of the weighted_gram capacity case -- one all +1, one +1 on the first L // 2 markers and
    -1 on the others -- under one weight q for every marker."""
    h = L // 2
    return np.array([[q * L, q * (h - (L - h))], [q * (h - (L - h)), q * L]], dtype=np.int64)
