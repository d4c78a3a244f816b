"""CPU: the numpy restatement of LD scores and the LD decay curve (include/eagle_hip.h section 1b'''v) pinned to plain loops.

r_api.ld_stats_host is what the device tests compare eagle_ld_stats / eagle_bed_ld_stats with; here it is compared with loops over
pairs that apply definitions 2 to 5 literally, in Python ints and floats.  Everything is an integer: every comparison is ==.  Also:
ld_band_host is the band ld_partners_host built inline (its output does not change), ld_half_decay on hand-made curves, and the
optional LD weight of grm_weights against a scalar loop.  No device work."""
import numpy as np
import pytest

N, L = 7, 40
WINDOWS = (1, 5, 39)
TWO30 = 1 << 30


def panel(seed=3):
    rng = np.random.default_rng(seed)
    G = rng.integers(-1, 2, size=(L, N)).astype(np.int8)
    G[11] = G[10]                                        # two identical markers: r2 = 1.0, u = 2^30 exactly
    G[20] = 1                                            # a monomorphic marker
    return G


def loops(band, chrom=None, pos=None, max_dist=0, edges=None):
    """Definitions 2 to 5, pair by pair."""
    Lb, W = len(band), len(band[0])
    U, cnt = [0] * Lb, [0] * Lb
    nb = 0 if edges is None else len(edges) - 1
    bsum, bpairs = [0] * nb, [0] * nb
    for i in range(Lb):
        for j in range(Lb):
            if not 1 <= abs(j - i) <= W:
                continue
            lo, hi = min(i, j), max(i, j)
            r2 = float(band[lo][hi - lo - 1])
            if not r2 >= 0.0:
                continue
            if chrom is not None and int(chrom[i]) != int(chrom[j]):
                continue
            d = abs(int(pos[j]) - int(pos[i])) if pos is not None else abs(j - i)
            if pos is not None and max_dist > 0 and d > max_dist:
                continue
            u = int(r2 * 1073741824.0)                   # an exact product; int() truncates
            U[i] += u
            cnt[i] += 1
            if i < j:
                for b in range(nb):
                    if int(edges[b]) <= d < int(edges[b + 1]):
                        bsum[b] += u
                        bpairs[b] += 1
    return U, cnt, bsum, bpairs


def same(got, want, with_bins):
    U, cnt = got[0], got[1]
    assert U.dtype == np.uint64 and cnt.dtype == np.int32
    assert [int(x) for x in U] == want[0] and [int(x) for x in cnt] == want[1]
    assert len(got) == (4 if with_bins else 2)
    if with_bins:
        assert got[2].dtype == np.uint64 and got[3].dtype == np.int64
        assert [int(x) for x in got[2]] == want[2] and [int(x) for x in got[3]] == want[3]


CHROM = (np.arange(L) >= 17).astype(np.int32) * 5 - (np.arange(L) >= 30)       # 0, 5, 4: a break at 17 and at 30, not sorted
POS = np.arange(L) * 1000 + np.where(np.arange(L) % 6 == 2, 3500, 0)             # not sorted: every sixth marker jumps past three


@pytest.mark.parametrize("window", WINDOWS)
def test_ld_stats_host_equals_loops_over_pairs(window):
    from eagleeverything_amd import r_api
    band = r_api.ld_band_host(panel(), window)
    per_offset = list(range(1, window + 2))
    cases = [
        dict(),
        dict(edges=per_offset),
        dict(chrom=CHROM),
        dict(chrom=CHROM, edges=per_offset),
        dict(pos=POS, max_dist=4200),                                           # cuts inside windows 5 and 39
        dict(pos=POS, max_dist=4200, edges=[500, 1500, 2600, 4000]),            # leaves pairs out at both ends (d = 500, d >= 4000)
        dict(pos=POS, edges=[0, 1, 1000, 1001, 5000, 1 << 40]),                 # pos without max_dist; a bin of one value
        dict(chrom=CHROM, pos=POS, max_dist=9000, edges=[2000, 3000, 8000]),
        dict(edges=[2, 4, 9]),                                                  # offsets 1 and >= 9 are in no bin
    ]
    for kw in cases:
        got = r_api.ld_stats_host(band, **kw)
        same(got, loops(band.tolist(), **kw), "edges" in kw)


def test_ld_stats_host_planted_markers():
    from eagleeverything_amd import r_api
    G = panel()
    band = r_api.ld_band_host(G, 5)
    assert band[10, 0] == 1.0                                                   # identical markers
    U, cnt, bsum, bpairs = r_api.ld_stats_host(band, edges=list(range(1, 7)))
    assert int(r_api.ld_stats_host(r_api.ld_band_host(G[10:12], 1))[0][0]) == TWO30
    assert U[20] == 0 and cnt[20] == 0                                          # monomorphic: no pair
    assert cnt[19] == 9 and cnt[25] == 9 and cnt[30] == 10                      # ... and it is nobody's partner
    without = np.delete(G, 20, axis=0)
    U2, cnt2 = r_api.ld_stats_host(r_api.ld_band_host(without, 39))
    U39, cnt39 = r_api.ld_stats_host(r_api.ld_band_host(G, 39))
    assert np.array_equal(np.delete(U39, 20), U2) and np.array_equal(np.delete(cnt39, 20), cnt2)      # it adds nothing to anyone
    score = 1.0 + U.astype(np.float64) * 2.0 ** -30
    assert score[20] == 1.0 and score[10] >= 2.0 and np.all(score >= 1.0) and np.all(score <= 1.0 + cnt)


@pytest.mark.parametrize("window", WINDOWS)
def test_ld_stats_host_sums_agree(window):
    from eagleeverything_amd import r_api
    band = r_api.ld_band_host(panel(5), window)
    U, cnt, bsum, bpairs = r_api.ld_stats_host(band, edges=[1, window + 1])     # one bin that covers every offset
    assert int(U.sum(dtype=np.uint64)) == 2 * int(bsum[0]) and int(cnt.sum()) == 2 * int(bpairs[0])
    U, cnt, bsum, bpairs = r_api.ld_stats_host(band, chrom=CHROM, edges=list(range(1, window + 2)))
    assert int(U.sum(dtype=np.uint64)) == 2 * int(bsum.sum(dtype=np.uint64))
    edges = [2, 3, 7]
    _, _, _, bpairs = r_api.ld_stats_host(band, chrom=CHROM, edges=edges)
    inside = sum(1 for i in range(L) for o in range(1, window + 1)
                 if i + o < L and band[i, o - 1] >= 0 and CHROM[i] == CHROM[i + o] and edges[0] <= o < edges[-1])
    assert int(bpairs.sum()) == inside


def test_ld_stats_host_refuses():
    from eagleeverything_amd import r_api
    band = r_api.ld_band_host(panel(), 5)
    for kw in (dict(chrom=CHROM[:-1]), dict(pos=POS[:-1]), dict(max_dist=5), dict(edges=[1]), dict(edges=[1, 1]), dict(edges=[3, 2, 5]),
               dict(edges=list(range(514)))):
        with pytest.raises(ValueError):
            r_api.ld_stats_host(band, **kw)
    assert len(r_api.ld_stats_host(band, edges=list(range(513)))) == 4          # 512 bins is the limit itself
    with pytest.raises(ValueError):
        r_api.ld_band_host(panel(), 257)


def old_ld_partners_host(Mt8, window, l, min_r2, chrom=None):
    """ld_partners_host as it was before ld_band_host was taken out of it."""
    from eagleeverything_amd import r_api
    G = np.asarray(Mt8)
    Lm, n = G.shape
    ch = None if chrom is None else np.asarray(chrom).ravel()
    F = G.astype(np.float64)
    Gi = G.astype(np.int64)
    s, q = Gi.sum(axis=1), (Gi * Gi).sum(axis=1)
    v = n * q - s * s
    vf = v.astype(np.float64)
    band = np.full((Lm, window), -1.0)
    for o in range(1, min(window, Lm - 1) + 1):
        d = np.rint(np.einsum("ij,ij->i", F[:-o], F[o:])).astype(np.int64)
        c = (n * d - s[:-o] * s[o:]).astype(np.float64)
        ok = (v[:-o] > 0) & (v[o:] > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            r2 = (c * c) / (vf[:-o] * vf[o:])
        band[:-o, o - 1] = np.where(ok, r2, -1.0)
    return band, r_api._ld_rank_band(band, l, min_r2, ch)


@pytest.mark.parametrize("window,l", [(1, 1), (5, 4), (39, 32), (256, 7)])
def test_ld_partners_host_is_unchanged_by_the_extraction(window, l):
    from eagleeverything_amd import r_api
    G = panel(9)
    for chrom, min_r2 in ((None, 0.0), (CHROM, 0.0), (None, 0.05)):
        band, (wp, wr) = old_ld_partners_host(G, window, l, min_r2, chrom)
        gp, gr = r_api.ld_partners_host(G, window, l, min_r2, chrom)
        assert gp.dtype == wp.dtype and np.array_equal(gp, wp) and np.array_equal(gr.view(np.uint64), wr.view(np.uint64))
        assert np.array_equal(r_api.ld_band_host(G, window).view(np.uint64), band.view(np.uint64))
    with pytest.raises(ValueError):
        r_api.ld_partners_host(G, 257, 1, 0.0)
    with pytest.raises(ValueError):
        r_api.ld_partners_host(G, 5, 33, 0.0)


def test_ld_half_decay_on_hand_made_curves():
    from eagleeverything_amd import r_api
    nan = float("nan")
    hd = r_api.ld_half_decay
    assert hd([1, 2, 3, 4, 5], [4, 4, 4, 4], [0.8, 0.5, 0.4, 0.1]) == 3         # 0.4 <= 0.4 is the first at most half
    assert hd([1, 2, 3, 4, 5], [4, 4, 4, 4], [0.8, 0.5, 0.41, 0.39]) == 4
    assert hd([1, 2, 3, 4, 5], [4, 4, 4, 4], [0.8, 0.7, 0.6, 0.5]) is None      # never halves
    assert hd([0, 100, 200, 300, 400], [0, 3, 0, 2], [nan, 0.6, nan, 0.3]) == 300     # empty bins are passed over; the first non-empty sets the level
    assert hd([0, 100, 200, 300, 400], [0, 3, 0, 2], [0.0, 0.6, 0.0, 0.31]) is None   # ... whatever their mean says
    assert hd([1, 2, 3], [0, 0], [nan, nan]) is None
    assert hd([5, 6, 7], [2, 2], [0.0, 0.0]) == 5                               # nothing to halve: the first non-empty bin itself
    assert hd([1, 2], [7], [0.9]) is None
    assert isinstance(hd([1, 2, 3], [1, 1], [0.5, 0.1]), int)
    with pytest.raises(ValueError):
        hd([1, 2, 3], [1, 1, 1], [0.5, 0.1, 0.0])


def counts(seed=1, Lm=60):
    rng = np.random.default_rng(seed)
    n0, n1, n2 = (rng.integers(0, 40, Lm) for _ in range(3))
    n0[3], n1[3] = 0, 0                                  # monomorphic
    n0[4], n1[4], n2[4] = 0, 0, 0                        # no call at all
    n0[5], n1[5], n2[5] = 99, 1, 0                       # a single copy of the rare allele
    return n0, n1, n2


@pytest.mark.parametrize("method", ["standardized", "vanraden1"])
def test_grm_weights_without_ld_score_keeps_every_bit(method):
    from eagleeverything_amd import r_api
    n0, n1, n2 = counts()
    inc = np.arange(n0.size) % 5 != 1
    for kw in (dict(), dict(maf=0.05), dict(maf=0.05, include=inc)):
        q0, s0, u0 = r_api.grm_weights(n0, n1, n2, method=method, **kw)
        q1, s1, u1 = r_api.grm_weights(n0, n1, n2, method=method, ld_score=None, **kw)
        assert q0.dtype == q1.dtype == np.uint32 and np.array_equal(q0, q1) and s0 == s1 and np.array_equal(u0, u1)
        if method == "vanraden1":
            assert s0 == 1.0 and set(q0.tolist()) <= {0, 1}
        else:                                            # all ones: dividing by 1.0 changes no bit
            q2, s2, u2 = r_api.grm_weights(n0, n1, n2, method=method, ld_score=np.ones(n0.size), **kw)
            assert np.array_equal(q0, q2) and s0 == s2 and np.array_equal(u0, u2)


@pytest.mark.parametrize("method", ["standardized", "vanraden1"])
def test_grm_weights_with_ld_score_equals_a_scalar_loop(method):
    from eagleeverything_amd import r_api
    n0, n1, n2 = counts(2)
    rng = np.random.default_rng(4)
    ls = 1.0 + rng.random(n0.size) * np.where(np.arange(n0.size) % 3 == 0, 512.0, 3.0)
    ls[7] = 1.0
    inc = np.arange(n0.size) % 7 != 2
    q, scale, used = r_api.grm_weights(n0, n1, n2, method=method, maf=0.02, include=inc, ld_score=ls)
    w = {}
    for m in range(n0.size):
        Nm = int(n0[m] + n1[m] + n2[m])
        c = int(2 * n2[m] + n1[m])
        den = c * (2 * Nm - c)
        if den > 0 and float(min(c, 2 * Nm - c)) >= 0.02 * float(2 * Nm) and inc[m]:
            w[m] = (((2.0 * float(Nm)) * float(Nm)) / float(den)) / float(ls[m]) if method == "standardized" else 1.0 / float(ls[m])
    assert sorted(w) == np.flatnonzero(used).tolist() and len(w) > 20
    want_scale = 2097151.0 / max(w.values())
    assert scale == want_scale
    for m in range(n0.size):
        assert int(q[m]) == (int(round(w[m] * want_scale)) if m in w else 0)    # round(): to nearest, ties to even, as rint
    assert int(q.max()) == 2097151 and q.dtype == np.uint32
    for bad in (ls[:-1], np.where(np.arange(ls.size) == 9, 0.999, ls), np.where(np.arange(ls.size) == 9, np.nan, ls)):
        with pytest.raises(ValueError):
            r_api.grm_weights(n0, n1, n2, method=method, ld_score=bad)


def test_grm_from_gram_vanraden1_with_ld_weights_is_the_weighted_ratio():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(8)
    n, Lm = 9, 30
    G = rng.integers(-1, 2, size=(n, Lm)).astype(np.int64)
    n0, n1, n2 = ((G == v).sum(axis=0) for v in (-1, 0, 1))
    ls = 1.0 + 4.0 * rng.random(Lm)
    q, scale, used = r_api.grm_weights(n0, n1, n2, method="vanraden1", ld_score=ls)
    Q = (G * q.astype(np.int64)[None, :]) @ G.T
    got = r_api.grm_from_gram(Q, {"method": "vanraden1", "scale": scale, "used": used, "q": q, "n0": n0, "n1": n1, "n2": n2})
    wq = q.astype(np.float64) / scale
    x = (G + 1).astype(np.float64)
    p = x.mean(axis=0) / 2.0
    Z = (x - 2.0 * p)[:, used]
    want = (Z * wq[used]) @ Z.T / np.sum(wq[used] * (2.0 * p * (1.0 - p))[used])
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
    plain = r_api.grm_weights(n0, n1, n2, method="vanraden1")
    Q1 = (G * plain[0].astype(np.int64)[None, :]) @ G.T
    info = {"method": "vanraden1", "scale": plain[1], "used": plain[2], "n0": n0, "n1": n1, "n2": n2}
    assert np.allclose(r_api.grm_from_gram(Q1, info), Z @ Z.T / np.sum((2.0 * p * (1.0 - p))[used]), rtol=1e-12, atol=1e-12)      # as before, without "q"
