"""Epistasis on the GPU: eagle_epistasis_loci / eagle_epistasis_pairs (k_epi_marker, k_epi_tile on the int8 MFMA) and the interface on
top (r_api.Epistasis, am.EpistasisOfLoci).

Expected values come from r_api.epistasis_host, the numpy restatement that tests/test_epistasis_host.py holds to plain loops and exact
fractions on the CPU.  Every comparison is exact: integers with array_equal, fp64 as bits (NaN and inf included)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

NS = (5, 16, 17, 127, 128, 129, 300)               # the 16-byte, 128-individual-chunk edges
LS = (1, 2, 127, 128, 129, 257, 400)               # the 32-block and 128-marker-tile edges
Y_EDGES = (63, -63, 64, -64, 65, -65, 8127, -8127, 8128, -8128, 8256, -8256, 1000000, -1000000, 0)      # the digit edges


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    """fp64 as bits, every NaN alike (the device writes one quiet NaN, numpy another)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(np.where(na, 0.0, a)), bits(np.where(nb, 0.0, b)))


def ingest(tmp, M8):
    from eagleeverything_amd import synth
    os.makedirs(str(tmp), exist_ok=True)
    return synth.write_geno_pair(str(tmp), np.ascontiguousarray(M8.T))


@functools.lru_cache(maxsize=None)
def case(n, L):
    """(M8, y, loci, host loci result, host all-pairs result at min_stat = -inf): read-only, computed once."""
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(1000 * n + L)
    M8 = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(n, L), p=[0.3, 0.4, 0.3])
    if L >= 127:
        M8[:, 40] = M8[:, 3]                        # a duplicate, its mirror and a monomorphic marker: undefined pairs
        M8[:, 41] = -M8[:, 3]
        M8[:, 90] = 1
    if L == 400:
        M8[:, 385:] = -1                            # the tile pair (markers 384 .., markers 384 ..) holds no defined pair, so no hit
    y = rng.integers(-1000000, 1000001, n).astype(np.int32)
    k = min(n, len(Y_EDGES))
    y[:k] = np.roll(Y_EDGES, LS.index(L) * 2 + NS.index(n))[:k]
    loci = rng.integers(0, L, 64)
    loci[0], loci[1], loci[5], loci[63] = 0, L - 1, loci[4], L - 1          # the first and the last marker, repeats
    host = r_api.epistasis_host(M8, y, loci=loci)
    pairs = r_api.epistasis_host(M8, y, min_stat=-math.inf)
    for a in (M8, y, loci, host["stat"], host["mom"], pairs["hit_ij"], pairs["hit_stat"], pairs["hit_mom"]):
        a.setflags(write=False)
    return M8, y, loci, host, pairs


def threshold(pairs):
    """The min_stat at which about 1 % of the defined pairs hit (0 where there are too few)."""
    st = pairs["hit_stat"]
    fin = st[np.isfinite(st)]
    return float(np.sort(fin)[int(0.99 * fin.size)]) if fin.size >= 100 else 0.0


def host_hits(pairs, min_stat):
    keep = pairs["hit_stat"] >= min_stat
    return pairs["hit_ij"][keep], pairs["hit_stat"][keep], pairs["hit_mom"][keep]


def check_pairs(got, pairs, min_stat, sel=None):
    """got = rcpp_api.epistasis_pairs' dict against the host's all-pairs table restricted to `sel` (a mask over it) at min_stat."""
    ij, st, mom = pairs["hit_ij"], pairs["hit_stat"], pairs["hit_mom"]
    if sel is not None:
        ij, st, mom = ij[sel], st[sel], mom[sel]
    keep = st >= min_stat
    assert got["ntested"] == st.size and got["nhits"] == int(keep.sum())
    assert np.array_equal(got["hit_ij"], ij[keep]) and same_bits(got["hit_stat"], st[keep]) and np.array_equal(got["hit_mom"], mom[keep])
    if st.size:
        top = st.max()
        first = ij[np.flatnonzero(st == top)[0]]
        assert got["max"][:2] == (int(first[0]), int(first[1])) and same_bits(got["max"][2], top)
    else:
        assert got["max"][:2] == (-1, -1) and math.isnan(got["max"][2])


# ------------------------------------------------------------------------------------------------ 1. both modes at the tile edges
@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_gpu_epistasis_loci_and_pairs_at_the_edges(tmp_path, n):
    from eagleeverything_amd import rcpp_api
    for L in LS:
        M8, y, loci, host, pairs = case(n, L)
        rcpp_api.drop_cache()
        geno = ingest(tmp_path / str(L), M8)
        Mt = geno["asciifileMt"]
        for k in (1, 2, 63, 64):
            stat, mom = rcpp_api.epistasis_loci(Mt, (n, L), y, loci[:k])
            assert stat.shape == (L, k) and mom.shape == (L, k, 5)
            assert np.array_equal(mom, host["mom"][:, :k]), (n, L, k)
            assert same_bits(stat, host["stat"][:, :k]), (n, L, k)
        assert np.isnan(stat[0, 0]) and np.isnan(stat[L - 1, 1])                     # i = j
        stat, mom = rcpp_api.epistasis_loci(Mt, (n, L), y, loci[:2], moments=False)
        assert mom is None and same_bits(stat, host["stat"][:, :2])
        t = threshold(pairs)
        got = rcpp_api.epistasis_pairs(Mt, (n, L), y, min_stat=t)
        check_pairs(got, pairs, t)
        if L >= 257 and n > 5:                                                       # the second pass skips a tile pair
            hij = got["hit_ij"]
            tiles = {(int(i) // 128, int(j) // 64) for i, j in hij}
            every = {(a, b) for a in range((L + 127) // 128) for b in range(2 * a, (L + 63) // 64)}
            assert 0 < got["nhits"] < pairs["ntested"] and tiles < every
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 2. the rules of the all-pairs mode
def raw_pairs(Mt, dims, y, chrom, gap, min_stat, cap, fill=-7):
    """eagle_epistasis_pairs through ctypes with sentinel-filled tables -> (rc, nhits, ntested, ij, stat, mom)."""
    from eagleeverything_amd import _lib, rcpp_api
    L = _lib.load()
    ctx = rcpp_api.context(0)
    i32, i64, dp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    ij, st, mom = np.full((cap, 2), fill, dtype=np.int32), np.full(cap, float(fill)), np.full((cap, 5), fill, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.int32)
    ch = None if chrom is None else np.ascontiguousarray(chrom, dtype=np.int32)
    nh, nt, mx = C.c_long(0), C.c_long(0), rcpp_api.EpiMax()
    rc = L.eagle_epistasis_pairs(ctx, os.fsencode(Mt), (C.c_long * 2)(*dims), yv.ctypes.data_as(i32), None if ch is None else ch.ctypes.data_as(i32),
                                 gap, min_stat, 8.0, ij.ctypes.data_as(i32), st.ctypes.data_as(dp), mom.ctypes.data_as(i64), cap, C.byref(nh),
                                 C.byref(nt), C.byref(mx))
    return rc, int(nh.value), int(nt.value), ij, st, mom


@pytest.mark.gpu
def test_gpu_epistasis_pairs_rules(tmp_path):
    from eagleeverything_amd import rcpp_api
    n, L = 128, 129
    M8, y, loci, host, pairs = case(n, L)
    rcpp_api.drop_cache()
    Mt = ingest(tmp_path, M8)["asciifileMt"]
    # min_stat = 0: every defined pair hits
    got = rcpp_api.epistasis_pairs(Mt, (n, L), y, min_stat=0.0)
    assert got["nhits"] == got["ntested"] == pairs["ntested"] < L * (L - 1) // 2
    check_pairs(got, pairs, 0.0)
    # -inf the same; +inf nothing (no pair of this panel is a perfect fit)
    check_pairs(rcpp_api.epistasis_pairs(Mt, (n, L), y, min_stat=-math.inf), pairs, -math.inf)
    none = rcpp_api.epistasis_pairs(Mt, (n, L), y, min_stat=math.inf)
    assert none["nhits"] == 0 and none["ntested"] == pairs["ntested"] and none["hit_ij"].shape == (0, 2)
    # hit_cap one below the total leaves the tables untouched; at the total they are written
    t = threshold(pairs)
    total = int((pairs["hit_stat"] >= t).sum())
    assert total > 3
    rc, nh, nt, ij, st, mom = raw_pairs(Mt, (n, L), y, None, 0, t, total - 1)
    assert rc == 0 and nh == total and nt == pairs["ntested"]
    assert (ij == -7).all() and (st == -7.0).all() and (mom == -7).all()
    rc, nh, nt, ij, st, mom = raw_pairs(Mt, (n, L), y, None, 0, t, total + 2)
    hij, hst, hmom = host_hits(pairs, t)
    assert rc == 0 and nh == total and np.array_equal(ij[:total], hij) and same_bits(st[:total], hst) and np.array_equal(mom[:total], hmom)
    assert (ij[total:] == -7).all() and (st[total:] == -7.0).all()
    short = rcpp_api.epistasis_pairs(Mt, (n, L), y, min_stat=t, hit_cap=0)
    assert short["nhits"] == total and short["hit_ij"] is None
    # gap = 3 with three chromosomes, and with one
    chrom = np.repeat([4, 9, 2], [50, 30, 49]).astype(np.int32)
    i, j = pairs["hit_ij"][:, 0].astype(np.int64), pairs["hit_ij"][:, 1].astype(np.int64)
    for ch, gap in ((chrom, 3), (None, 3), (chrom, 1000)):
        sel = ~((j - i <= gap) & (np.ones(i.size, dtype=bool) if ch is None else ch[i] == ch[j]))
        assert 0 < sel.sum() < sel.size or ch is None
        check_pairs(rcpp_api.epistasis_pairs(Mt, (n, L), y, chrom=ch, gap=gap, min_stat=t), pairs, t, sel)
    # a perfect fit is +inf, a hit at every threshold and the maximum
    yi = M8[:, 7].astype(np.int32) * M8[:, 100]                                       # y = g_i g_j exactly
    hp = rcpp_api.epistasis_pairs(Mt, (n, L), yi, min_stat=math.inf)
    assert hp["max"] == (7, 100, math.inf) and [7, 100] in hp["hit_ij"].tolist() and np.all(np.isinf(hp["hit_stat"]))
    stat, _ = rcpp_api.epistasis_loci(Mt, (n, L), yi, [100, 7])
    assert stat[7, 0] == math.inf and stat[100, 1] == math.inf and np.isnan(stat[7, 1])
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 3. sources
@pytest.mark.gpu
def test_gpu_epistasis_streamed_equals_resident_and_pairs_need_residence(tmp_path, monkeypatch):
    from eagleeverything_amd import r_api, rcpp_api
    from eagleeverything_amd._lib import EagleError
    n, L = 300, 2600                                                                  # 512 padded bytes a row: 1.3 MB
    rng = np.random.default_rng(5)
    M8 = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(n, L), p=[0.25, 0.5, 0.25])
    y = rng.integers(-1000000, 1000001, n).astype(np.int32)
    loci = np.concatenate(([0, L - 1, 511, 512, 513, 513], rng.integers(0, L, 58)))
    rcpp_api.drop_cache()
    Mt = ingest(tmp_path, M8)["asciifileMt"]
    stat, mom = rcpp_api.epistasis_loci(Mt, (n, L), y, loci)
    host = r_api.epistasis_host(M8, y, loci=loci)
    assert np.array_equal(mom, host["mom"]) and same_bits(stat, host["stat"])
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.001")                          # 1 MB: the image goes in row windows
    s2, m2 = rcpp_api.epistasis_loci(Mt, (n, L), y, loci)
    assert np.array_equal(m2, mom) and np.array_equal(bits(s2), bits(stat))
    with pytest.raises(EagleError) as e:
        rcpp_api.epistasis_pairs(Mt, (n, L), y, min_stat=50.0)
    assert e.value.code == -3 and "prune or filter" in e.value.text
    monkeypatch.delenv("EAGLE_HIP_MAX_RESIDENT_GB")
    rcpp_api.drop_cache()


@pytest.mark.gpu
def test_gpu_epistasis_on_view_alias(golden, tmp_path):
    from eagleeverything_amd import am, r_api, rcpp_api
    M8 = golden("geno_150x100")["M8"]
    n, L = M8.shape
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    na = np.array([1, 2, 57, 130, 150])                                               # 1-based, as R hands them over
    kept = np.setdiff1d(np.arange(n), na - 1)
    view = am.reshape_geno(geno, na, view=True)
    assert list(view["dim_of_ascii_M"]) == [n - 5, L]
    sub = np.ascontiguousarray(M8[kept])
    y = np.random.default_rng(6).integers(-1000000, 1000001, n - 5).astype(np.int32)
    loci = [5, 99, 0]
    host = r_api.epistasis_host(sub, y, loci=loci)
    assert not same_bits(host["stat"], r_api.epistasis_host(M8[5:], y, loci=loci)["stat"])      # which individuals are kept matters
    stat, mom = rcpp_api.epistasis_loci(view["asciifileMt"], (n - 5, L), y, loci)
    assert np.array_equal(mom, host["mom"]) and same_bits(stat, host["stat"])
    pairs = r_api.epistasis_host(sub, y, min_stat=-math.inf)
    t = threshold(pairs)
    check_pairs(rcpp_api.epistasis_pairs(view["asciifileMt"], (n - 5, L), y, min_stat=t), pairs, t)
    rcpp_api.drop_cache()


# ------------------------------------------------------------------------------------------------ 4. the Python layer
@pytest.mark.gpu
def test_gpu_epistasis_python_layer(golden, tmp_path):
    from scipy import special
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    M8 = golden("geno_150x100")["M8"]
    n, L = M8.shape
    rng = np.random.default_rng(7)
    a, b = 49, 85                                                                    # the pair of the panel whose product is least in the span of its factors
    y = rng.standard_normal(n)
    y = y + 0.3 * (y.max() - y.min()) * M8[:, a] * M8[:, b]
    rcpp_api.drop_cache()
    geno = ingest(tmp_path, M8)
    yq, scale = r_api.quantise_trait(y)
    # all pairs: the planted pair is the maximum and a hit at the default p
    res = r_api.Epistasis(geno, y)
    pairs = r_api.epistasis_host(M8, yq, min_stat=res["min_stat"])
    assert res["scale"] == scale and res["min_stat"] == float(special.fdtri(1.0, n - 4.0, 1.0 - 1e-8))
    assert res["max"][:2] == (a, b) and res["nhits"] == pairs["nhits"] >= 1 and res["ntested"] == pairs["ntested"]
    assert np.array_equal(res["hits"], pairs["hit_ij"]) and same_bits(res["stat"], pairs["hit_stat"]) and np.array_equal(res["mom"], pairs["hit_mom"])
    k = res["hits"].tolist().index([a, b])
    assert np.array_equal(res["p"], special.fdtrc(1.0, n - 4.0, res["stat"])) and res["p"][k] < 1e-8
    # b3 and its standard error against the least-squares fit of the quantised trait, in trait units
    Xd = np.column_stack([np.ones(n), M8[:, a], M8[:, b], M8[:, a] * M8[:, b]]).astype(np.float64)
    yr = yq / scale
    coef = np.linalg.lstsq(Xd, yr, rcond=None)[0]
    rss = float(((yr - Xd @ coef) ** 2).sum())
    se = math.sqrt(rss / (n - 4) * np.linalg.inv(Xd.T @ Xd)[3, 3])
    assert abs(res["b3"][k] - coef[3]) <= 1e-9 * abs(coef[3]) and abs(res["se"][k] - se) <= 1e-9 * se
    assert abs((res["b3"][k] / res["se"][k]) ** 2 - res["stat"][k]) <= 1e-9 * res["stat"][k]
    # an integer trait is used as it is; loci mode is dense; more than 64 loci take two calls
    lv = np.arange(L)[::-1][:70]
    rl = r_api.Epistasis(geno, yq, loci=lv)
    host = r_api.epistasis_host(M8, yq, loci=lv)
    assert rl["scale"] == 1.0 and rl["stat"].shape == (L, 70) and same_bits(rl["stat"], host["stat"]) and np.array_equal(rl["mom"], host["mom"])
    assert same_bits(rl["stat"][a, L - 1 - b], res["stat"][k]) and np.isnan(rl["p"][a, L - 1 - a])
    # gap and map
    chrom = ["1"] * 50 + ["2"] * 50
    rg = r_api.Epistasis(geno, y, map={"Chr": chrom, "Pos": list(range(L)), "SNP": ["m%d" % i for i in range(L)]}, gap=L, min_stat=0.0)
    assert rg["ntested"] <= 2500 and rg["nhits"] == rg["ntested"] and all(i < 50 <= j for i, j in rg["hits"])
    # the loci AM() reports, on the conditional residual, with missing records
    Mt8 = np.ascontiguousarray(M8.T)
    yt = 1.5 * (M8[:, 20] + M8[:, 60]) + rng.standard_normal(n)
    na = rng.choice(n, 10, replace=False)
    yt[na] = np.nan
    X = np.ones((n, 1))
    am_res = am.AM(yt, X, geno, maxit=3)
    assert len(am_res["selected_loci"]) >= 1
    eo = am.EpistasisOfLoci(am_res, yt, X, geno)
    kk = len(am_res["selected_loci"])
    assert eo["selected_loci"] == [int(j) for j in am_res["selected_loci"]] and eo["loci"].tolist() == [int(j) - 1 for j in am_res["selected_loci"]]
    assert eo["stat"].shape == (L, kk) and list(eo["geno"]["dim_of_ascii_M"]) == [n - 10, L]
    eff = am.MarkerEffects(am_res, yt, X, geno)
    pq, _ = r_api.quantise_trait(eff["Py"])
    kept = np.setdiff1d(np.arange(n), na)
    assert same_bits(eo["stat"], r_api.epistasis_host(M8[kept], pq, loci=eo["loci"])["stat"])
    fin = np.isfinite(eo["stat"])
    assert all(np.isnan(eo["stat"][j, c]) for c, j in enumerate(eo["loci"])) and fin.sum() > L * kk // 2       # the panel holds duplicates
    assert np.all((eo["p"][fin] >= 0) & (eo["p"][fin] <= 1)) and np.isnan(eo["p"][~fin]).all()
    rcpp_api.drop_cache()
