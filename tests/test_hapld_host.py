"""CPU: the numpy restatement of the pairwise haplotype EM (r_api.hap_ld_host, include/eagle_hip.h section 1b''''vii), the block
partition (r_api.hap_blocks_host) and sets_from_blocks against tests/hapld_truth.py: counting loops, a scalar loop of the rule with ==,
the same EM in mpmath at 40 digits, closed forms, and brute-force partitions.  No device work."""
import functools

import numpy as np
import pytest

import hapld_truth as T

TOL = 1e-10


@functools.lru_cache(maxsize=None)
def panel(name):
    from eagleeverything_amd import synth
    if name == "mosaic":
        Mt8 = T.founder_mosaic(120, 90)
    else:
        Mt8 = synth.genotypes_marker_major(int(name), 300)
    Mt8.setflags(write=False)
    return Mt8


@functools.lru_cache(maxsize=None)
def host(name, window):
    from eagleeverything_amd import r_api
    return r_api.hap_ld_host(panel(name), window)


# ------------------------------------------------------------------------------------------------ 1. the table
def test_cells_from_the_six_sums_equal_counting():
    from eagleeverything_amd import r_api
    Mt8 = panel("65")
    n = Mt8.shape[1]
    for i, j in ((0, 1), (3, 43), (17, 24), (100, 140), (298, 299)):
        si, qi, sj, qj, d, e, f, h = T.pair_sums(Mt8[i], Mt8[j])
        c = r_api.hap_ld_cells(n, si, qi, sj, qj, d, e, f, h)
        N = T.count_cells(Mt8[i], Mt8[j])
        for a in range(3):
            for b in range(3):
                assert int(c["N%d%d" % (a, b)]) == N[a][b], (i, j, a, b)
        assert sum(map(sum, N)) == n


# ------------------------------------------------------------------------------------------------ 2. the rule, with ==
@pytest.mark.parametrize("name,window,rows", [("257", 40, range(0, 260, 9)), ("65", 40, range(0, 260, 7)), ("mosaic", 12, range(0, 78, 3)),
                                              ("3", 5, range(0, 295, 11))])
def test_hap_ld_host_equals_the_scalar_loop(name, window, rows):
    Mt8, res = panel(name), host(name, window)
    L = Mt8.shape[0]
    seen = iterated = 0
    for i in rows:
        for o in (1, 7, window) if window >= 7 else (1, window):
            j = i + o
            want = T.scalar_rule(Mt8[i], Mt8[j]) if j < L else None
            at = (i, o - 1)
            if want is None:
                assert res["dprime"][at] == -2.0 and res["r2"][at] == -1.0 and not T.bit(res["recomb"], i, j) and not T.bit(res["strong"], i, j)
                continue
            seen += 1
            iterated += want["iterations"] > 0
            assert res["pBB"][at] == want["pBB"] and res["dprime"][at] == want["dprime"] and res["r2"][at] == want["r2"], (i, j)
            assert res["pmin"][at] == want["pmin"] and res["iterations"][at] == want["iterations"] and res["code"][at] == want["code"]
            assert T.bit(res["recomb"], i, j) == want["recomb"] and T.bit(res["strong"], i, j) == want["strong"]
    assert seen >= 20 and (iterated >= 5 or name == "3")
    d = res["dprime"]
    defined = d > -2.0
    assert res["counts"].tolist() == [int(defined.sum()), int(res["code"].sum()), sum(T.bit(res["recomb"], i, i + o) for i in range(L) for o in range(1, window + 1)),
                                      int((defined & (np.abs(d) >= 0.8)).sum())]


def test_a_pair_stopped_at_max_iter_has_code_1():
    from eagleeverything_amd import r_api
    Mt8 = panel("65")
    res = r_api.hap_ld_host(Mt8, 7, max_iter=3)
    late = np.argwhere(host("65", 40)["iterations"][:, :7] > 3)
    assert late.shape[0] > 50 and res["counts"][1] == late.shape[0]
    for i, c in late[:40]:
        want = T.scalar_rule(Mt8[i], Mt8[i + c + 1], max_iter=3)
        assert want["code"] == 1 and want["iterations"] == 3 and res["code"][i, c] == 1 and res["iterations"][i, c] == 3
        assert res["dprime"][i, c] == want["dprime"] and res["r2"][i, c] == want["r2"]
    assert res["iterations"].max() == 3


# ------------------------------------------------------------------------------------------------ 3. the fixed point at 40 digits
def test_fixed_point_against_mpmath():
    """Where the EM contracts with rho <= 0.9, |p_k - p*| <= rho / (1 - rho) delta_k <= 9 tol; 64 ulps of 1 cover the roundings of one
    step.  D' and r2_h follow to first order: dD = dp, d(D') = dp / Dmax, d(r2) = 2 |D| dp / den.  Pairs with rho > 0.9 are left out;
    at most 5 % may be."""
    eps = 9 * TOL + 64 * 2.0 ** -53
    used = left_out = 0
    for name, window, rows in (("257", 40, range(0, 260, 13)), ("65", 40, range(0, 260, 13)), ("mosaic", 12, range(0, 78, 4))):
        Mt8, res = panel(name), host(name, window)
        for i in rows:
            for o in (1, 7, window):
                if res["dprime"][i, o - 1] == -2.0:
                    continue
                tr = T.mp_fixed_point(Mt8[i], Mt8[i + o])
                if tr["rho"] > 0.9:
                    left_out += 1
                    continue
                used += 1
                at = (i, o - 1)
                assert res["code"][at] == 0
                assert abs(res["pBB"][at] - tr["pBB"]) <= eps, (name, i, o)
                small = abs(tr["D"]) <= eps                              # the sign of D, and with it the branch of Dmax, is not settled
                dmax = float(tr["dmax_least"] if small else tr["dmax"])
                assert abs(res["dprime"][at] - tr["dprime"]) <= (2 if small else 1) * eps / dmax * (1 + 1e-9) + 16 * 2.0 ** -53, (name, i, o)
                assert abs(res["r2"][at] - tr["r2"]) <= (2 * float(abs(tr["D"])) * eps + eps * eps) / float(tr["den"]) * (1 + 1e-9) + 16 * 2.0 ** -53
    assert used >= 150 and left_out <= 0.05 * (used + left_out), (used, left_out)


# ------------------------------------------------------------------------------------------------ 4. closed forms
def test_closed_forms():
    """n = 64: 2n is a power of two, so every allele frequency and every product of two of them is exact in fp64, and the closed forms
    hold to the last bit.  At other n the products p p and p q round, and identical markers keep D' = 1 and r2_h = 1 only to that
    rounding: see test_identical_markers_at_any_n."""
    from eagleeverything_amd import r_api, synth
    rng = np.random.default_rng(4)
    n = 64
    base = synth.genotypes_marker_major(n, 6, seed=8)
    hom = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int8)           # no het: x = 0 with every partner
    hom[:3] = (1, -1, 1)
    hap = rng.random((4, 2 * n)) < 0.5                                   # two markers drawn as independent haplotypes, twice
    ind = [(h[0::2].astype(np.int8) + h[1::2] - 1).astype(np.int8) for h in hap]
    Mt8 = np.stack([base[0], base[0], -base[0], hom, base[1], ind[0], ind[1], np.zeros(n, np.int8) + 1, ind[2], ind[3]])
    res = r_api.hap_ld_host(Mt8, 9)
    # x = 0: the counting estimate, no iteration
    for j in (4, 5, 6):
        N = T.count_cells(Mt8[3], Mt8[j])
        assert N[1][1] == 0 and res["iterations"][3, j - 4] == 0 and res["code"][3, j - 4] == 0
        assert res["pBB"][3, j - 4] == (2 * N[2][2] + N[2][1] + N[1][2]) / (2.0 * n)
    # identical polymorphic markers: D' = 1, r2_h = 1 exactly, the two mixed haplotypes are never seen
    assert res["dprime"][0, 0] == 1.0 and res["r2"][0, 0] == 1.0 and res["pmin"][0, 0] == 0.0
    assert T.bit(res["strong"], 0, 1) and not T.bit(res["recomb"], 0, 1)
    # a marker and its negation: D' = -1.  pBB, the frequency the stop rule watches, is the one that dies out here, quadratically
    # (pBB' = x t / T with t <= pBB pAA / (pBA pAB)): a last step below tol leaves it below 18 tol^2, not at 0.
    assert res["dprime"][0, 1] == -1.0 and res["dprime"][1, 0] == -1.0 and res["r2"][0, 1] == 1.0 and res["pmin"][1, 0] <= 1e-15
    # independent haplotypes: all four gametes
    assert T.bit(res["recomb"], 5, 6) and T.bit(res["recomb"], 8, 9) and res["pmin"][5, 0] > 0.1 and abs(res["dprime"][5, 0]) < 0.5
    # a monomorphic marker: undefined from both sides
    assert (res["dprime"][7] == -2.0).all() and (res["r2"][7] == -1.0).all() and not res["recomb"][7].any() and not res["strong"][7].any()
    assert all(res["dprime"][7 - o, o - 1] == -2.0 for o in range(1, 8))
    # beyond the panel's end
    assert (res["dprime"][9] == -2.0).all() and res["dprime"][8, 0] > -2.0 and (res["dprime"][8, 1:] == -2.0).all()
    # one individual: nothing is defined
    one = r_api.hap_ld_host(np.zeros((5, 1), dtype=np.int8), 3)
    assert one["counts"].tolist() == [0, 0, 0, 0] and (one["dprime"] == -2.0).all()
    with pytest.raises(ValueError):
        r_api.hap_ld_host(Mt8, 257)


def test_identical_markers_at_any_n():
    """pBB converges to p exactly (the mixed haplotypes die out quadratically: 1 - t = pBA^2 / den), so D = p - fl(p p) and
    Dmax = fl(p q): half an ulp of 1 on p p, relative to D = p q, and three relative roundings (p q, the quotient, D itself).  r2_h
    squares D and divides by fl(p q)^2: twice that, and three more roundings.  The negated marker gives -1 and 1 exactly at every n:
    there D = -fl(p_i p_j) and Dmax is the same product."""
    from eagleeverything_amd import r_api, synth
    u = 2.0 ** -53
    for n in (3, 65, 90, 257):
        base = synth.genotypes_marker_major(n, 40, seed=n)
        base = base[[m for m in range(40) if 0 < n + int(base[m].sum()) < 2 * n]][:8]
        Mt8 = np.concatenate([np.stack([g, g, -g]) for g in base])
        res = r_api.hap_ld_host(Mt8, 2)
        for m in range(0, Mt8.shape[0], 3):
            p = (n + int(Mt8[m].sum())) / (2.0 * n)
            bound = 0.5 * u / (p * (1.0 - p)) + 4 * u
            assert 1.0 - bound <= res["dprime"][m, 0] <= 1.0 and abs(res["r2"][m, 0] - 1.0) <= 2 * bound + 4 * u, (n, m)
            assert res["pmin"][m, 0] == 0.0 and res["pBB"][m, 0] == p
            assert res["dprime"][m, 1] == -1.0 and res["dprime"][m + 1, 0] == -1.0 and res["r2"][m, 1] == 1.0 and res["pmin"][m, 1] <= 1e-15


# ------------------------------------------------------------------------------------------------ 5. blocks
def random_pairs(rng, L, window, share):
    return {(i, j) for i in range(L) for j in range(i + 1, min(L, i + window + 1)) if rng.random() < share}


@pytest.mark.parametrize("method", ["fourgamete", "spine"])
def test_hap_blocks_host_equals_brute_force(method):
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(9)
    L = 70
    chrom = np.array(["1"] * 23 + ["2"] * 30 + ["X"] * 17)
    pos = np.cumsum(rng.integers(100, 3000, L))
    nonempty = 0
    for window, share, kw in ((5, 0.08, {}), (12, 0.03, dict(chrom=chrom)), (12, 0.03, dict(chrom=chrom, pos=pos, kb=9)), (70, 0.01, {}),
                              (3, 0.0, dict(chrom=chrom)), (12, 0.03, dict(min_snp=4)), (1, 0.3, {}), (12, 0.03, dict(min_snp=1))):
        rec = random_pairs(rng, L, window, share)
        strong = random_pairs(rng, L, window, 1.0 - 2 * share)
        want = T.blocks_brute(rec, strong, L, window, method=method, **kw)
        first, last, block_of = r_api.hap_blocks_host(T.mask_from_pairs(rec, L, window), T.mask_from_pairs(strong, L, window), window, method=method, **kw)
        assert list(zip(first.tolist(), last.tolist())) == want, (window, share, sorted(kw))
        exp = np.full(L, -1)
        for b, (f, e) in enumerate(want):
            exp[f:e + 1] = b
            assert e - f + 1 <= window + 1 and e - f + 1 >= kw.get("min_snp", 2)
            if "chrom" in kw:
                assert chrom[f] == chrom[e]
            if "kb" in kw:
                assert pos[e] - pos[f] <= 9000
        assert np.array_equal(block_of, exp)
        nonempty += len(want) > 0
    assert nonempty >= 6
    # the window limit: without any objection a block holds window + 1 markers
    none = np.zeros((L, 1), dtype=np.uint64)
    full = T.mask_from_pairs({(i, j) for i in range(L) for j in range(i + 1, min(L, i + 5))}, L, 4)
    first, last, _ = r_api.hap_blocks_host(none, full, 4, method=method)
    assert (last - first + 1).tolist() == [5] * 14
    with pytest.raises(ValueError):
        r_api.hap_blocks_host(none, full, 4, method="gabriel")
    with pytest.raises(ValueError):
        r_api.hap_blocks_host(none, full, 4, kb=5)                          # kb needs positions


def test_planted_blocks_are_found_and_a_monomorphic_marker_joins():
    from eagleeverything_amd import r_api
    Mt8, bounds = T.planted_blocks()
    L = Mt8.shape[0]
    res = r_api.hap_ld_host(Mt8, 50)
    for (f, e), (f2, _) in zip(bounds, bounds[1:]):
        assert T.bit(res["recomb"], e, f2) and f2 == e + 1                 # a recombinant pair across every boundary
    for f, e in bounds:
        assert not any(T.bit(res["recomb"], i, j) for i in range(f, e + 1) for j in range(i + 1, e + 1))
    first, last, block_of = r_api.hap_blocks_host(res["recomb"], res["strong"], 50, method="fourgamete")
    assert list(zip(first.tolist(), last.tolist())) == bounds and (block_of >= 0).all()
    mono = np.array(Mt8)
    mono[bounds[1][0] + 3] = 1                                            # inside the second block
    res = r_api.hap_ld_host(mono, 50)
    first, last, _ = r_api.hap_blocks_host(res["recomb"], res["strong"], 50)
    assert list(zip(first.tolist(), last.tolist())) == bounds
    first, last, _ = r_api.hap_blocks_host(res["recomb"], res["strong"], 50, method="spine")       # an undefined pair is not STRONG
    assert (bounds[1][0], bounds[1][1]) not in list(zip(first.tolist(), last.tolist()))


# ------------------------------------------------------------------------------------------------ 6. sets
def test_sets_from_blocks_cuts_and_names():
    from eagleeverything_amd import r_api
    tab = {"first": np.array([0, 10, 200]), "last": np.array([4, 159, 263]), "chrom": ["1", "1", "2"]}
    out = r_api.sets_from_blocks({"blocks": tab})
    assert out["names"] == ["1:0-4", "1:10-159/1", "1:10-159/2", "1:10-159/3", "2:200-263"]
    assert [s.tolist() for s in out["sets"]] == [list(range(0, 5)), list(range(10, 74)), list(range(74, 138)), list(range(138, 160)), list(range(200, 264))]
    assert all(s.dtype == np.int64 and s.size <= 64 for s in out["sets"])
    out = r_api.sets_from_blocks(tab, max_markers=3, names=["a", "b", "c"])
    assert out["names"][:3] == ["a/1", "a/2", "b/1"] and out["sets"][1].tolist() == [3, 4] and len(out["sets"]) == 2 + 50 + 22
    assert r_api.sets_from_blocks({"first": [2], "last": [3]})["names"] == ["2-3"]
    assert r_api.sets_from_blocks({"first": [], "last": []}) == {"sets": [], "names": []}
    for bad in (dict(max_markers=65), dict(max_markers=0), dict(names=["a"])):
        with pytest.raises(ValueError):
            r_api.sets_from_blocks(tab, **bad)
    with pytest.raises(ValueError):
        r_api.sets_from_blocks({"first": [5], "last": [4]})
