"""CPU: the restated launch arithmetic of tests/marker_regimes_truth.py against the source text of the kernels and launchers, and its
builders against plain loops and r_api's restatements, so that tests/test_gpu_marker_regimes.py asserts the regimes the library really
has and compares against a truth that is right.  No device work."""
import os
import re

import numpy as np
import pytest

import marker_regimes_truth as R
from conftest import ROOT


def source(name):
    return open(os.path.join(ROOT, "eagleeverything_amd", "csrc", name)).read()


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def body(text, start, stop="\n}\n"):
    a = text.index(start)
    return text[a:text.index(stop, a)]


def test_constants_are_the_source_text():
    k, load, ing, i8, score, h = (source(f) for f in ("eagle_kernels.hip", "eagle_load.cpp", "eagle_ingest.cpp", "eagle_i8mfma.hip",
                                                      "eagle_score.hip", "eagle_t8.h"))
    # a staging buffer: every staged reader and writer cuts at 67,108,864 bytes
    assert "(long)(%d / std::max(1L, ncols))" % R.STAGE_BYTES in load and "(long)std::min(budget, %d.0)" % R.STAGE_BYTES in load
    assert "(long)h.row_bytes, p.runs, w.nb, stride, %d, threads" % R.STAGE_BYTES in load and "(w.nb + 15) / 16 * 16" in load
    assert "std::min(nrows, cap_bytes / stride)" in load
    assert "(long)(%d / std::max(1L, stride))" % R.STAGE_BYTES in ing and "(long)(%d / in_stride)" % R.STAGE_BYTES in ing
    assert "long w = (long)(%d / out_stride) / 256 * 256;" % R.STAGE_BYTES in ing
    # the row bands
    for name in ("eagle_dev_decode_ascii", "eagle_dev_encode_ascii", "eagle_dev_pack2b", "eagle_dev_unpack2b"):
        b = body(k, 'extern "C" int %s(' % name)
        assert "r0 += %d)" % R.BAND_ROWS in b and "rows - r0 < %d ? rows - r0 : %d" % (R.BAND_ROWS, R.BAND_ROWS) in b, name
    b = body(k, 'extern "C" int eagle_dev_decode_ascii(')
    assert "raw + r0 * line_stride" in b and "out + r0 * ld_out" in b
    b = body(k, 'extern "C" int eagle_dev_encode_ascii(')
    assert "in + r0 * ld_in" in b and "out + r0 * (cols + 1)" in b
    b = body(k, 'extern "C" int eagle_dev_pack2b(')
    assert "in + r0 * ld_in" in b and "out + r0 * row_bytes" in b
    b = body(k, 'extern "C" int eagle_dev_unpack2b(')
    assert "raw + r0 * stride" in b and "out + r0 * ld_out" in b
    b = body(k, 'extern "C" int eagle_dev_transpose_i8(')
    assert "r0 += 64L * 65535)" in b and "in + r0 * ld_in, ld_in, out + r0," in b and R.TRANSPOSE_BAND_ROWS == 64 * 65535
    b = body(i8, 'extern "C" int eagle_dev_pack_fp4(')
    assert "r0 < L_pad; r0 += %d)" % R.BAND_ROWS in b and "Mt8 + r0 * ld" in b and "(uint8_t*)Mt4 + r0 * (n_pad / 2)" in b
    # the arg-max
    b = body(k, 'extern "C" int eagle_dev_tsq_argmax(')
    assert "int nparts = (int)((L + 255) / 256);" in b and "if (nparts > %d) nparts = %d;" % (R.ARGMAX_BLOCKS, R.ARGMAX_BLOCKS) in b
    assert b.count("dim3(nparts), dim3(%d)" % R.ARGMAX_THREADS) == 2 and "(long*)(block_scratch + 1024)" in b
    assert k.count("i < L; i += (long)gridDim.x * 256") == 2 and "v > bv || (v == bv && i < bi)" in k
    assert "isinf(mx) ? mx : mx - fabs(mx) * 1e-9" in k and "if (t == t && t >= thr) cnt++;" in k
    # the line scores
    assert "#define SCORE_CHUNK_TILES %dL" % R.SCORE_CHUNK_TILES in score and "#define T8 %d " % R.T8 in h
    assert "t0 += SCORE_CHUNK_TILES" in score and "img + r0 * ld" in score and "out + r0 * T);" in score and "r0 = t0 * T8" in score
    assert "rowsB * ld, 0x00020000" in score and "(double)ld * T8 >= 2147483648.0" in score
    # the grid-stride copies
    assert k.count("(total + 255) / 256 < %d ? (total + 255) / 256 : %d" % (R.PACK2_GRID_CAP, R.PACK2_GRID_CAP)) == 2
    assert "const long total = L_pad * (ld >> 4);" in k and "idx < total; idx += (long)gridDim.x * 256" in k
    assert "k_add_i32, dim3(%d), dim3(256)" % R.ADD_GRID in k and "dst, src, count / 4);" in k and "i < count4; i += (long)gridDim.x * 256" in k
    # the capacities
    hh = header()
    assert int(re.search(r"#define\s+EAGLE_WGRAM_MAX_MARKERS\s+(\d+)L", hh).group(1)) == R.WGRAM_MAX_MARKERS == (2 ** 31 - 1) // 127
    assert int(re.search(r"#define\s+EAGLE_SCORES_MAX_LINE\s+(\d+)L", hh).group(1)) == R.SCORES_MAX_LINE == (2 ** 23 - 1) // 128 * 128
    assert int(re.search(r"#define\s+EAGLE_SCORES_MAX_WEIGHT\s+(\d+)L", hh).group(1)) == R.SCORES_MAX_WEIGHT
    assert "if (q[m] >= (1u << 21))" in ing and R.WGRAM_MAX_WEIGHT == 127 * (1 + 128 + 128 * 128)
    assert re.search(r"static inline long stream_chunk_rows_core\(size_t budget, long row_bytes, long total_rows_pad\) \{\s*"
                     r"if \(budget == \(size_t\)-1\) budget = \(size_t\)8 << 30;\s*"
                     r"long rows = \(long\)\(budget / 2 / \(size_t\)row_bytes\) / 256 \* 256;\s*if \(rows < 256\) rows = 256;", source("eagle_host.h"))


def test_regime_arithmetic_by_hand():
    assert R.ARGMAX_ONE_TRIP == R.SCORE_CHUNK_LINES == 262144 and R.PACK2_ONE_TRIP == 16777216 and R.ADD_ONE_TRIP == 2097152
    assert 127 * R.WGRAM_MAX_MARKERS == 2 ** 31 - 8 and 127 * (R.WGRAM_MAX_MARKERS + 1) >= 2 ** 31
    assert 256 * R.SCORES_MAX_LINE == 2147450880 < 2 ** 31 <= 256 * (R.SCORES_MAX_LINE + 128) and 128 * R.SCORES_MAX_LINE < 2 ** 31
    # n = 37: a line of 38 bytes, a sidecar row of 10 bytes staged at 16; n = 1,003: 1,004 and 251 at 256
    assert R.text_rows_per_chunk(37) == 1766022 and R.sidecar_rows_per_chunk(37) == 4194304
    assert R.text_rows_per_chunk(1003) == 66841 and R.sidecar_rows_per_chunk(1003) == 262144
    assert R.text_rows_per_chunk(1023) == 65536 and R.text_rows_per_chunk(1024) == 65472      # "about 1 KiB or shorter"
    assert R.mt_window_lines(37) == 1765888 and R.mt_window_lines(1003) == 66816 and R.mt_window_lines(7) == 8388608
    assert R.bands(65535) == [(0, 65535)] and R.bands(65536) == [(0, 65535), (65535, 1)] and R.bands(65537)[1] == (65535, 2)
    assert R.bands(196700) == [(0, 65535), (65535, 65535), (131070, 65535), (196605, 95)]
    assert R.chunk_bands(196700, 66841) == [(0, 65535), (65535, 1306), (66841, 65535), (132376, 1306), (133682, 63018)]
    assert R.chunk_bands(100, 40) == [(0, 40), (40, 40), (80, 20)]
    assert [R.argmax_grid(L) for L in (1, 255, 256, 257, 262144, 262145, 1000003)] == [(1, 1), (1, 1), (1, 1), (2, 1), (1024, 1), (1024, 2), (1024, 4)]
    assert [R.score_chunks(L) for L in (1, 262143, 262144, 262145, 600011)] == [1, 1, 1, 2, 3]
    assert R.pack2_grid(16, 256) == (1, 1) and R.pack2_grid(1048576, 256) == (65536, 1) and R.pack2_grid(1048592, 256) == (65536, 2)
    assert R.pack2_grid(R.pad(16777300), 256) == (65536, 17)
    assert [R.add_trips(c) for c in (4, 2097152, 2097156, 2 ** 22 + 4, 2 ** 29 + 4)] == [1, 1, 2, 3, 257]
    assert R.stream_window(10 ** 9, 256, R.pad(R.WGRAM_MAX_MARKERS)) == 1953024 and R.stream_window(1000, 256, 5120) == 256
    assert R.stream_window(8 << 30, 256, 512) == 512
    for P in R.PERIODS:                   # prime, and no divisor of the edges the panels are meant to straddle
        assert all(P % d for d in range(2, int(P ** 0.5) + 1)) and all(e % P for e in (65535, 256, 1024, 262144))


@pytest.mark.parametrize("P,n,L", [(5, 3, 23), (7, 37, 7), (11, 1, 30)])
def test_periodic_builders_by_plain_loops(tmp_path, P, n, L):
    from eagleeverything_amd import synth
    base = R.base_panel(P, n, seed=P)
    assert base.dtype == np.int8 and base.shape == (P, n) and set(np.unique(base).tolist()) <= {-1, 0, 1}
    assert (base[0] == -1).all() and (base[1] == 0).all() and (base[2] == 1).all()
    planted = np.array([1, L - 2, L - 1])
    g = R.periodic_lines(base, L, planted)
    for m in range(L):
        want = [((m // 3 ** (j % min(n, 19))) % 3) - 1 for j in range(n)] if m in planted else base[m % P].tolist()
        assert g[m].tolist() == want, m
    path = str(tmp_path / "Mt.ascii")
    rows = R.write_periodic(path, base, L, planted)
    assert np.array_equal(rows, g[planted])
    assert open(path, "rb").read() == open(synth.write_ascii(str(tmp_path / "ref.ascii"), g), "rb").read()
    assert open(path, "rb").read() == R.text_of(g).tobytes()
    per_line = np.arange(3 * P).reshape(P, 3)
    got = R.expand(per_line, L, planted, np.array([[-1, -2, -3]] * 3))
    for m in range(L):
        assert got[m].tolist() == ([-1, -2, -3] if m in planted else per_line[m % P].tolist())
    assert np.array_equal(R.counts_of(g), np.array([[(row == v).sum() for v in (-1, 0, 1)] for row in g]))


def test_planted_lines_differ_from_their_neighbours_and_the_base():
    for n in (20, 37, 1003):                # (3^7 lines of 7 genotypes are too few for this to hold at n = 7)
        base = R.base_panel(1021, n, seed=n)
        at = R.planted_markers(196700, 1021)
        assert at.tolist() == [3, 65534, 65535, 65536, 131069, 131070, 131071, 196604, 196605, 196606, 196699]
        rows = [R.planted_line(m, n) for m in at.tolist()]
        assert len({r.tobytes() for r in rows}) == len(rows)
        for m, r in zip(at.tolist(), rows):                                     # not the line it replaces, nor one beside it
            assert all((r != base[(m + o) % 1021]).any() for o in (-1, 0, 1)), (n, m)
    at = R.planted_markers(600011, 1021, edges=(R.SCORE_CHUNK_LINES,))
    assert at.tolist() == [3, 262143, 262144, 262145, 524287, 524288, 524289, 600010]
    assert R.planted_markers(65535, 1021).tolist() == [3, 65534] and R.planted_markers(65536, 1021).tolist() == [3, 65534, 65535]


def test_packed_rows_by_plain_loops():
    rng = np.random.default_rng(1)
    for cols in (1, 4, 7, 37):
        g = rng.integers(-1, 2, size=(5, cols)).astype(np.int8)
        got = R.pack2b_rows(g)
        assert got.shape == (5, 16) == (5, R.sidecar_row_bytes(cols))
        for r in range(5):
            for b in range(16):
                assert got[r, b] == sum((int(g[r, 4 * b + q]) + 1) << (2 * q) for q in range(4) if 4 * b + q < cols)
    assert R.sidecar_row_bytes(1003) == 256 and R.sidecar_row_bytes(64) == 16 and R.sidecar_row_bytes(65) == 32
    assert "return ((cols + 3) / 4 + 15) / 16 * 16;" in source("eagle_host.h")
    g = rng.integers(-1, 2, size=(3, 32)).astype(np.int8)
    got = R.fp4_rows(g)
    code = {-1: 0xA, 0: 0x0, 1: 0x2}
    assert got.shape == (3, 16) and all(got[r, k] == code[int(g[r, 2 * k])] | code[int(g[r, 2 * k + 1])] << 4 for r in range(3) for k in range(16))


def test_tsq_truth_is_the_oracles_rule(oracle):
    rng = np.random.default_rng(2)
    for L in (1, 5, 300):
        a, v = rng.standard_normal(L), rng.uniform(0.5, 2.0, L)
        if L >= 5:
            a[[1, 3]], v[[1, 3]] = 7.0, 0.25                                   # an exact tie: the first wins
            a[0], v[0] = 0.0, 0.0                                              # NaN in front of it
        t, idx, mx, near = R.tsq_truth(a, v)
        t_o, idx_o, mx_o = oracle.tsq_argmax(a, v)                             # 1-based
        assert idx + 1 == idx_o and mx == mx_o and np.array_equal(t, t_o, equal_nan=True)
        assert near == (2 if L >= 5 else 1)
    t, idx, mx, near = R.tsq_truth(np.zeros(4), np.zeros(4))
    assert idx == -1 and np.isnan(mx) and near == 0 and np.isnan(t).all()
    t, idx, mx, near = R.tsq_truth([1.0, 2.0, 0.0, 3.0], [1.0, 0.0, 0.0, 0.0])
    assert idx == 1 and mx == np.inf and near == 2


@pytest.mark.parametrize("L", [1, 255, 256, 257, 262145])
def test_argmax_cases_select_what_they_are_built_to_select(L):
    names = set(R.argmax_plants(L))
    assert {"last", "all_nan"} <= names and (("trips" in names) == (L > 262144)) and (("blocks" in names) == (L >= 257))
    for name in names:
        a, vara, want = R.argmax_case(L, name)
        t, idx, mx, near = R.tsq_truth(a, vara)
        assert idx == want, (L, name)
        peak, nan, inf = R.argmax_plants(L)[name]
        if name == "all_nan":
            assert idx == -1 and near == 0
            continue
        assert mx == (np.inf if inf else 100.0) and near == (len(inf) if inf else len(peak) + (1 if L > 2 else 0)), (L, name)
        if nan:
            assert np.isnan(t[nan]).all()
        if name == "last":
            assert idx == L - 1
        if name == "trips":
            assert sorted(peak) == [idx, idx + R.ARGMAX_ONE_TRIP]              # one thread, two trips
        if name == "lanes":
            assert peak[0] // 64 == peak[1] // 64
        if name == "waves":
            assert peak[0] // 256 == peak[1] // 256 and peak[0] // 64 != peak[1] // 64
        if name == "blocks":
            assert len({p // 256 for p in peak}) >= 2


def test_capacity_truths_by_int64_products():
    from eagleeverything_amd import r_api
    d = R.score_digits([R.SCORE_FULL_DIGITS, -R.SCORES_MAX_WEIGHT, R.SCORES_MAX_WEIGHT, 0, 127, -129])
    assert d[:, 0].tolist() == [-128, -128, -128, -63] and d[:, 1].tolist() == [0, 0, 0, -64] and d[:, 2].tolist() == [0, 0, 0, 64]
    assert d[:, 4].tolist() == [127, 0, 0, 0] and d[:, 5].tolist() == [127, -1, 0, 0] and abs(R.SCORE_FULL_DIGITS) <= R.SCORES_MAX_WEIGHT
    w = R.capacity_score_tile(5, 13, seed=1)
    assert np.array_equal(r_api.score_digits_host(w), R.score_digits(w))
    assert R.score_digits(w).any(axis=(1, 2)).all() and (w[0] == R.SCORE_FULL_DIGITS).all() and (w[1] == -2 ** 30).all()
    g = np.stack([np.full(13, -1), np.random.default_rng(3).integers(-1, 2, 13)]).astype(np.int8)
    for C in (13, 14, 40, 100):
        reps = -(-C // 13)
        full_w, full_g = np.tile(w, (1, reps))[:, :C], np.tile(g, (1, reps))[:, :C]
        assert np.array_equal(R.tiled_scores(w, g, C), r_api.line_scores_host(full_g, full_w))
    for L in (2, 7, 10):
        G = np.ones((2, L), dtype=np.int64)
        G[1, L // 2:] = -1
        assert np.array_equal(R.wgram_capacity_truth(L, 5), (G * 5) @ G.T)
    Q = R.wgram_capacity_truth(R.WGRAM_MAX_MARKERS, R.WGRAM_MAX_WEIGHT)
    assert Q[0, 1] == 0 and Q[0, 0] == Q[1, 1] == R.WGRAM_MAX_WEIGHT * R.WGRAM_MAX_MARKERS < 2 ** 52
