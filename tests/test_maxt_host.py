"""CPU: r_api.maxt_host / maxt_permutations_host / maxt_key64_host (the numpy restatement of include/eagle_hip.h section 1b''''vi that
the GPU tests compare the device with) against tests/maxt_truth.py's plain loops on Python ints, and MaxT's statistics built from the
raw words against CaseControl's trend test and exact fractions.  No device work."""
from fractions import Fraction

import numpy as np
import pytest

import maxt_truth as truth

KEYS = ("d_obs", "V", "key_obs", "count1", "maxkey", "argmax")


def panel(n, L, seed):
    from eagleeverything_amd import synth
    return synth.genotypes_marker_major(n, L, seed=seed)


def same(host, want, L, R):
    assert host["d_obs"].dtype == np.int64 and host["V"].dtype == np.int64 and host["count1"].dtype == np.int32
    assert host["key_obs"].dtype == np.float64 and host["maxkey"].dtype == np.float64 and host["argmax"].dtype == np.int32
    assert host["d_obs"].shape == (L,) and host["maxkey"].shape == (R,)
    for k in KEYS:
        a = np.asarray(want[k], dtype=host[k].dtype)
        if a.dtype == np.float64:
            assert np.array_equal(host[k].view(np.uint64), a.view(np.uint64)), k
        else:
            assert np.array_equal(host[k], a), k


def test_mixer_gives_the_published_splitmix64_words():
    from eagleeverything_amd import r_api
    for j, word in enumerate(truth.SPLITMIX64_FROM_ZERO):
        assert truth.mix64(0, 0, j) == word
    k = r_api.maxt_key64_host(0, 0, 4)
    assert k.dtype == np.uint64 and [int(v) for v in k] == [((w >> 32) << 16) | j for j, w in enumerate(truth.SPLITMIX64_FROM_ZERO)]
    # a seed that wraps, a large ordinal, strata in the top 16 bits
    for seed, r in ((2 ** 64 - 1, 1), (0x0123456789ABCDEF, 2 ** 31 - 1), (7, 1000000)):
        st = [0, 65535, 3, 3, 65535]
        got = r_api.maxt_key64_host(seed, r, 5, st)
        assert [int(v) for v in got] == [truth.key64(seed, r, j, st[j]) for j in range(5)]
        assert len(set(int(v) for v in got)) == 5


@pytest.mark.parametrize("N", [3, 5, 64, 70, 1000])
def test_rows_are_permutations_that_stay_inside_their_strata(N):
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(N)
    strata = rng.integers(0, 4, N) * 1000
    for st in (None, strata):
        P = r_api.maxt_permutations_host(N, st, 11, 5, 6)
        assert P.dtype == np.int32 and P.shape == (6, N)
        for q in range(6):
            assert P[q].tolist() == truth.permutation(N, st, 11, 5 + q)
            assert sorted(P[q].tolist()) == list(range(N))
            if st is not None:
                assert np.array_equal(st[P[q]], st)
        assert N < 5 or len({tuple(r) for r in P.tolist()}) > 1
    ident = r_api.maxt_permutations_host(N, np.arange(N)[::-1], 3, 1, 4)            # one individual per stratum
    assert np.array_equal(ident, np.tile(np.arange(N), (4, 1)))
    # a call depends on (seed, first, R) alone: rows of a later call are the rows of the longer one
    assert np.array_equal(r_api.maxt_permutations_host(N, strata, 11, 8, 3), r_api.maxt_permutations_host(N, strata, 11, 5, 6)[3:])


@pytest.mark.parametrize("n,L", [(5, 7), (16, 9), (33, 12), (70, 10)])
def test_counts_and_maxima_against_loops(n, L):
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(10 * n + L)
    Mt8 = panel(n, L, n)
    Mt8[L - 1] = 1                                                          # monomorphic: V = 0, key = 0, count1 = R
    Mt8[L - 2] = Mt8[1]                                                     # a duplicate: equal words, the tie goes to marker 1
    used = np.ones(n, dtype=bool)
    used[rng.integers(0, n, max(1, n // 6))] = False
    if used.sum() < 3:
        used[:3] = True
    strata = rng.integers(0, 3, n)
    R = 9
    for t in (rng.integers(0, 2, n), rng.integers(-1000000, 1000001, n)):
        t[np.flatnonzero(used)[:2]] = (t[np.flatnonzero(used)[0]], t[np.flatnonzero(used)[0]] + 1)       # never constant
        t = np.clip(t, -1000000, 1000000)
        for um, st in ((None, None), (used, None), (used, strata)):
            want = truth.maxt(Mt8.tolist(), t.tolist(), None if um is None else um.tolist(), None if st is None else st.tolist(), 42, 3, R)
            host = r_api.maxt_host(Mt8, t, um, st, 42, 3, R)
            same(host, want, L, R)
            assert want["V"][L - 1] == 0 and host["key_obs"][L - 1] == 0.0 and host["count1"][L - 1] == R
            assert host["count1"][L - 2] == host["count1"][1] and host["d_obs"][L - 2] == host["d_obs"][1]
            assert not np.any(host["argmax"] == L - 2)
            for m in range(L):                                              # two roundings of the exact ratio
                e = want["exact"][m]
                assert abs(Fraction(float(host["key_obs"][m])) - e) <= e * Fraction(3, 2 ** 53)
    N = int(used.sum())
    perm = np.stack([np.arange(N), np.arange(N)[::-1], rng.permutation(N)])
    want = truth.maxt(Mt8.tolist(), t.tolist(), used.tolist(), None, 0, 1, 3, perm=perm.tolist())
    host = r_api.maxt_host(Mt8, t, used, strata, 99, 1, 3, perm=perm)        # seed and strata are ignored with perm
    same(host, want, L, 3)
    assert np.array_equal(host["count1"] >= 1, np.ones(L, dtype=bool))       # the identity always reaches the observed value
    assert host["maxkey"][0] == host["key_obs"].max() and host["argmax"][0] == int(np.argmax(host["key_obs"]))


def test_digit_edges_choose_the_planes():
    from eagleeverything_amd import r_api
    for tmax, P in ((1, 1), (127, 1), (128, 2), (16383, 2), (16384, 3), (1000000, 3)):
        t = np.array([tmax, -tmax, 0, 1, -1, tmax - 1, 1 - tmax])
        got_P, pl = r_api.maxt_digit_planes(t)
        assert got_P == P == truth.planes(tmax) and pl.dtype == np.int8 and pl.shape == (P, t.size)
        for k, v in enumerate(t.tolist()):
            d = truth.digits(v)
            assert pl[:, k].tolist() == d[:P] and not any(d[P:]) and all(-127 <= x <= 127 for x in d)
            assert d[0] + 128 * d[1] + 16384 * d[2] == v
    # the pass itself at those edges: int64 sums do not depend on the planes
    n, L = 21, 6
    Mt8 = panel(n, L, 3)
    for tmax in (127, 128, 16383, 16384, 1000000):
        t = np.zeros(n, dtype=np.int64)
        t[[0, 5, n - 1]] = (tmax, -tmax, tmax)
        same(r_api.maxt_host(Mt8, t, None, None, 1, 1, 4), truth.maxt(Mt8.tolist(), t.tolist(), None, None, 1, 1, 4), L, 4)


def test_split_invariance_of_first_and_R():
    from eagleeverything_amd import r_api
    n, L = 40, 15
    Mt8 = panel(n, L, 8)
    t = np.random.default_rng(8).integers(-500, 500, n)
    st = np.arange(n) % 3
    whole = r_api.maxt_host(Mt8, t, None, st, 5, 1, 20)
    a, b = r_api.maxt_host(Mt8, t, None, st, 5, 1, 7), r_api.maxt_host(Mt8, t, None, st, 5, 8, 13)
    assert np.array_equal(a["count1"] + b["count1"], whole["count1"])
    assert np.array_equal(np.concatenate([a["maxkey"], b["maxkey"]]), whole["maxkey"])
    assert np.array_equal(np.concatenate([a["argmax"], b["argmax"]]), whole["argmax"])
    for k in ("d_obs", "V", "key_obs"):
        assert np.array_equal(a[k], whole[k]) and np.array_equal(b[k], whole[k])
    ra, rb = (r_api.maxt_from_raw(x, t, "qt", 1.0, f) for x, f in ((a, 1), (b, 8)))
    m, w = r_api.maxt_merge(ra, rb), r_api.maxt_from_raw(whole, t, "qt", 1.0, 1)
    assert m["R"] == 20 and m["first"] == 1
    for k in ("count1", "count2", "emp1", "emp2", "max_stat", "argmax", "stat", "p"):
        assert np.array_equal(m[k], w[k], equal_nan=True), k
    with pytest.raises(ValueError):
        r_api.maxt_merge(ra, ra)


def test_maxt_statistics_on_a_case_control_trait():
    """stat is CaseControl's trend chi-square: both are a handful of correctly rounded fp64 operations on the same exact integers."""
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(5)
    n, L, R = 90, 40, 200
    Mt8 = panel(n, L, 5)
    Mt8[7] = 0                                                              # monomorphic
    status = rng.integers(0, 2, n).astype(np.float64)
    status[[4, 50]] = np.nan
    liab = Mt8[3].astype(np.float64) * 2.5 + rng.standard_normal(n)          # a planted strong marker
    status = np.where(np.isnan(status), np.nan, (liab > 0).astype(np.float64))
    t, used, strata, kind, scale = r_api.maxt_trait(status)
    assert kind == "cc" and scale == 1.0 and strata is None and used.sum() == n - 2 and set(t[used].tolist()) == {0, 1}
    raw = r_api.maxt_host(Mt8, t, used, None, 17, 1, R)
    res = r_api.maxt_from_raw(raw, t[used], kind, scale)
    lab = np.where(used, t, -1)
    cc = r_api.case_control_from_counts(r_api.group_counts_host(Mt8, lab, 2))
    ok = np.arange(L) != 7
    assert np.all(np.abs(res["stat"][ok] - cc["trend"][ok]) <= 1e-12 * cc["trend"][ok])
    assert np.all(np.abs(res["p"][ok] - cc["p_trend"][ok]) <= 1e-9 * cc["p_trend"][ok])
    for k in ("stat", "p", "beta", "r2", "emp1", "emp2"):
        assert np.isnan(res[k][7]) and not np.any(np.isnan(res[k][ok])), k
    assert np.all(res["emp2"][ok] >= res["emp1"][ok]) and np.all(res["count2"] >= res["count1"] - (~ok) * R)
    assert res["count2"][3] == 0 and res["emp2"][3] == 1.0 / (R + 1) and res["argmax"].shape == (R,)
    assert res["n_used"] == n - 2 and res["R"] == R and res["kind"] == "cc"
    assert np.array_equal(res["count2"], [(raw["maxkey"] >= k).sum() for k in raw["key_obs"]])
    N = n - 2
    assert np.array_equal(res["max_stat"], N * (raw["maxkey"] / float(N * int((t[used] ** 2).sum()) - int(t[used].sum()) ** 2)))
    # one label per individual: every permutation is the identity
    t2, used2, strata2, _, _ = r_api.maxt_trait(status, within=["id%d" % i for i in range(n)])
    r1 = r_api.maxt_host(Mt8, t2, used2, strata2, 17, 1, 12)
    assert np.array_equal(r1["count1"], np.full(L, 12)) and np.all(r1["maxkey"] == raw["key_obs"].max())


def test_maxt_statistics_on_a_quantitative_trait():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(6)
    n, L = 60, 25
    Mt8 = panel(n, L, 6)
    y = rng.standard_normal(n) + 0.9 * Mt8[2]
    y[[1, 30]] = np.nan
    t, used, strata, kind, scale = r_api.maxt_trait(y, within=np.arange(n) % 2)
    assert kind == "qt" and np.abs(t).max() <= 1000000 and strata.dtype == np.int32
    res = r_api.maxt_from_raw(r_api.maxt_host(Mt8, t, used, strata, 1, 1, 50), t[used], kind, scale)
    g, yy = Mt8[:, used].astype(np.float64), y[used]
    for m in (0, 2, 11):                                                    # ordinary least squares in floating point
        A = np.stack([np.ones(g.shape[1]), g[m]], axis=1)
        b, rss = np.linalg.lstsq(A, yy, rcond=None)[:2]
        F = (np.sum((yy - yy.mean()) ** 2) - rss[0]) / (rss[0] / (g.shape[1] - 2))
        assert abs(res["beta"][m] - b[1]) <= 1e-5 * max(1.0, abs(b[1])) and abs(res["stat"][m] - F) <= 1e-4 * max(1.0, F)
    assert np.all(res["emp2"] >= res["emp1"]) and res["kind"] == "qt" and res["scale"] == scale
    for bad in (dict(trait=[1.0, np.nan, np.nan, 0.0]), dict(trait=[2.0, 2.0, 2.0, 2.0]), dict(trait=[0, 1, 2, 3], kind="cc"),
                dict(trait=[0, 1, 0, 1], kind="x"), dict(trait=[0.0, 1.0, 0.0, 1.0], within=[1, None, 2, 1]),
                dict(trait=[0.0, 1.0, 0.0, 1.0], within=[1, 2, 1])):
        with pytest.raises(ValueError):
            r_api.maxt_trait(**bad)
