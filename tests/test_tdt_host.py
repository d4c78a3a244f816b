"""CPU: the numpy restatement of the transmission disequilibrium test (r_api.tdt_host, include/eagle_hip.h section 1b''''viii) against the
definition in plain loops over allele choices (tests/tdt_truth.py), its symmetries, the family and sign rules of the flips, and the
statistics of r_api.tdt_summary on exact integers.  No device work."""
import itertools
import math

import numpy as np
import pytest

import mendel_truth as M
import tdt_truth as T


def test_all_64_code_triples_match_the_enumeration_of_allele_choices():
    from eagleeverything_amd import r_api
    table = T.triple_table()
    triples = sorted(table)
    g, called = np.zeros((64, 3), dtype=np.int8), np.ones((64, 3), dtype=bool)
    for x, t in enumerate(triples):
        M.plant(g, called, (2, 0, 1), x, t)
    got = r_api.tdt_host(g, called, [(2, 0, 1)])
    T.same(got, T.tdt_loops(g, called, [(2, 0, 1)]), "64 triples")
    for x, t in enumerate(triples):
        assert tuple(got["marker"][x]) == table[t][:5], t
    # of the 27 called triples 11 are informative; het parents = PT + PU + MT + MU + 2 W on every triple; incomplete triples give nothing
    assert len(T.informative_triples()) == 11
    for t, (pt, pu, mt, mu, w, comp, hf, hm) in table.items():
        assert hf + hm == pt + pu + mt + mu + 2 * w, t
        if 3 in t or t in M.error_triples():
            assert (pt, pu, mt, mu, w, comp, hf, hm) == (0,) * 8, t
    assert got["trio"][0].tolist() == [sum(v[5] for v in table.values()), sum(v[6] for v in table.values()), sum(v[7] for v in table.values()),
                                       sum(v[0] + v[2] + v[4] for v in table.values()), sum(v[1] + v[3] + v[4] for v in table.values()),
                                       sum(v[4] for v in table.values())]
    # on the image a not-called code is a het
    as_het = r_api.tdt_host(g, None, [(2, 0, 1)])
    T.same(as_het, T.tdt_loops(g, None, [(2, 0, 1)]), "64 triples as hets")
    assert as_het["trio"][0, 0] > got["trio"][0, 0]


@pytest.mark.parametrize("miss", (0.0, 0.1))
def test_pedigree_with_planted_mendel_errors_matches_the_loops(miss):
    from eagleeverything_amd import r_api
    g, called, trios = M.pedigree(12, 20, 90, seed=5, miss=miss)
    g, called = g.copy(), called.copy()
    errs = [t for t in M.error_triples() if 3 not in t]
    planted = []
    for k, x in enumerate(range(0, 90, 7)):
        trio = trios[k % trios.shape[0]]
        M.plant(g, called, trio, x, errs[k % len(errs)])
        planted.append((k % trios.shape[0], x))
    lst = np.concatenate((trios, trios[:3], [[int(trios[0, 0]), -1, int(trios[0, 2])], [int(trios[1, 0]), -1, -1]])).astype(np.int32)
    cm = called if miss > 0 else None
    want = T.tdt_loops(g, cm, lst, seed=3, first=2, R=7)
    got = r_api.tdt_host(g, cm, lst, seed=3, first=2, R=7)
    T.same(got, want, miss)
    assert got["marker"].sum() > 100 and got["count1"].max() <= 7 and (got["trio"][-2:] == 0).all()       # an unknown parent: nothing
    assert np.array_equal(got["trio"][:3], got["trio"][20:23])                                             # a trio listed twice counts twice
    # the errored markers of a trio contribute nothing to it: alone in the list it has an empty row there
    for k, x in planted[:4]:
        one = r_api.tdt_host(g, cm, lst[k:k + 1])
        assert (one["marker"][x] == 0).all()
        base = r_api.tdt_host(np.delete(g, x, axis=0), None if cm is None else np.delete(cm, x, axis=0), lst[k:k + 1])
        assert np.array_equal(one["trio"], base["trio"])


def test_swapping_the_alleles_swaps_t_and_u_and_keeps_the_keys():
    from eagleeverything_amd import r_api
    g, called, trios = M.pedigree(10, 30, 70, seed=9, miss=0.05)
    a = r_api.tdt_host(g, called, trios, seed=11, R=9)
    b = r_api.tdt_host(-g, called, trios, seed=11, R=9)
    assert np.array_equal(a["marker"][:, [1, 0, 3, 2, 4]], b["marker"]) and np.array_equal(a["trio"][:, [0, 1, 2, 4, 3, 5]], b["trio"])
    for k in ("key_obs", "count1", "maxkey", "argmax"):
        assert np.array_equal(a[k], b[k]), k
    assert a["marker"][:, 4].sum() > 0 and not np.array_equal(a["marker"][:, 0], a["marker"][:, 1])


def test_sibs_flip_together_and_family_joins_couples():
    from eagleeverything_amd import r_api
    trios = np.asarray([(4, 0, 1), (5, 2, 3), (6, 0, 1), (7, 2, 3), (8, 0, 3), (9, 0, -1), (10, 0, -1)], dtype=np.int32)
    fam = r_api.tdt_families(trios)
    assert fam.tolist() == [0, 1, 0, 1, 4, 5, 5] == T.families(trios.tolist()) and fam.dtype == np.int32
    s = r_api.tdt_signs_host(fam, 17, 1, 200)
    assert s.shape == (200, 7) and set(np.unique(s).tolist()) == {-1, 1}
    assert np.array_equal(s[:, 0], s[:, 2]) and np.array_equal(s[:, 1], s[:, 3]) and not np.array_equal(s[:, 0], s[:, 1])
    assert s.tolist() == [[T.sign(17, 1 + q, phi) for phi in fam.tolist()] for q in range(200)]
    assert 60 < (s[:, 0] < 0).sum() < 140
    joined = r_api.tdt_signs_host([3, 3, 3, 3, 9, 9, 2], 17, 1, 50)
    assert (joined[:, :4] == joined[:, :1]).all() and np.array_equal(joined[:, 4], joined[:, 5])
    # the same through tdt_host: joining every couple into one family makes every flip +-d_obs, so count1 = R
    g, called, tr = M.pedigree(6, 12, 40, seed=2)
    one = r_api.tdt_host(g, None, tr, family=np.zeros(12, dtype=np.int32), seed=1, R=20)
    assert (one["count1"] == 20).all() and (one["maxkey"] == one["key_obs"].max()).all()
    T.same(one, T.tdt_loops(g, None, tr, family=[0] * 12, seed=1, R=20), "one family")
    own = r_api.tdt_host(g, None, tr, family=np.arange(12, dtype=np.int32) * 5000, seed=1, R=20)
    T.same(own, T.tdt_loops(g, None, tr, family=[5000 * k for k in range(12)], seed=1, R=20), "own families")
    assert (own["count1"] < 20).any()


def test_flip_ranges_add_and_concatenate():
    from eagleeverything_amd import r_api
    g, called, trios = M.pedigree(10, 25, 60, seed=4, miss=0.02)
    whole = r_api.tdt_host(g, called, trios, seed=5, first=1, R=30)
    a, b = r_api.tdt_host(g, called, trios, seed=5, first=1, R=13), r_api.tdt_host(g, called, trios, seed=5, first=14, R=17)
    assert np.array_equal(a["count1"] + b["count1"], whole["count1"])
    assert np.array_equal(np.concatenate([a["maxkey"], b["maxkey"]]), whole["maxkey"])
    assert np.array_equal(np.concatenate([a["argmax"], b["argmax"]]), whole["argmax"])
    merged = r_api.tdt_merge(r_api.tdt_summary(a, 1), r_api.tdt_summary(b, 14))
    ref = r_api.tdt_summary(whole, 1)
    assert sorted(merged) == sorted(ref)
    for k in ref:
        assert np.array_equal(merged[k], ref[k], equal_nan=True), k
    with pytest.raises(ValueError):
        r_api.tdt_merge(r_api.tdt_summary(a, 1), r_api.tdt_summary(b, 10))       # overlapping ordinals
    none = r_api.tdt_host(g, called, trios)
    assert none["maxkey"].size == 0 and (none["count1"] == 0).all() and np.array_equal(none["key_obs"], whole["key_obs"])


def test_summary_hand_table_exact_p_and_parent_of_origin():
    from scipy import special

    from eagleeverything_amd import r_api
    mk = np.asarray([[20, 5, 10, 5, 0], [3, 1, 2, 4, 6], [0, 0, 0, 0, 0], [4, 0, 0, 0, 0], [0, 0, 0, 5, 2]], dtype=np.int32)
    Tm, Um = mk[:, 0] + mk[:, 2] + mk[:, 4], mk[:, 1] + mk[:, 3] + mk[:, 4]
    with np.errstate(all="ignore"):
        key = np.where(Tm + Um > 0, ((Tm - Um) * (Tm - Um)).astype(np.float64) / (Tm + Um), 0.0)
    raw = {"marker": mk, "trio": np.zeros((1, 6), dtype=np.int32), "key_obs": key, "count1": np.zeros(5, dtype=np.int32),
           "maxkey": np.zeros(0), "argmax": np.zeros(0, dtype=np.int32)}
    s = r_api.tdt_summary(raw)
    assert (s["T"][0], s["U"][0], s["chisq"][0], s["or"][0]) == (30, 10, 10.0, 3.0)
    assert s["p"][0] == special.chdtrc(1.0, 10.0) and "emp1" not in s and s["R"] == 0
    for x in range(5):
        t, u = int(Tm[x]), int(Um[x])
        if t + u == 0:
            assert all(np.isnan(s[k][x]) for k in ("chisq", "p", "or", "p_exact", "chisq_pat", "chisq_mat", "z_poo", "p_poo"))
            continue
        tail = sum(math.comb(t + u, k) for k in range(min(t, u) + 1)) / 2.0 ** (t + u)
        assert s["p_exact"][x] == pytest.approx(min(1.0, 2.0 * tail), rel=1e-12)
    assert s["p_exact"][1] == 1.0                        # T = 11, U = 11: twice the lower tail exceeds 1
    assert s["or"][3] == np.inf and s["or"][4] == pytest.approx(2.0 / 7.0)
    # the parental chi-squares leave W out; z_poo by its formula
    assert s["chisq_pat"][0] == 225.0 / 25.0 and s["chisq_mat"][0] == 25.0 / 15.0 and np.isnan(s["chisq_pat"][4]) and s["chisq_mat"][4] == 5.0
    p1, p2, pp = 20 / 25, 10 / 15, 30 / 40
    z = (p1 - p2) / math.sqrt(pp * (1 - pp) * (1 / 25 + 1 / 15))
    assert s["z_poo"][0] == pytest.approx(z, rel=1e-14) and s["p_poo"][0] == pytest.approx(math.erfc(abs(z) / math.sqrt(2.0)), rel=1e-12)
    assert np.isnan(s["z_poo"][3])                       # no maternal transmission: undefined
    # emp1 / emp2 as MaxT defines them
    raw.update(count1=np.asarray([0, 3, 4, 4, 1], dtype=np.int32), maxkey=np.asarray([1.0, 10.0, 12.0, 0.5]), argmax=np.zeros(4, dtype=np.int32))
    s = r_api.tdt_summary(raw, first=7)
    assert s["emp1"][0] == 1 / 5 and s["emp1"][1] == 4 / 5 and np.isnan(s["emp1"][2]) and (s["R"], s["first"]) == (4, 7)
    assert s["count2"][0] == 2 and s["emp2"][0] == 3 / 5 and np.array_equal(s["max_stat"], raw["maxkey"])


def ascertained(seed, causal=17):
    """60 couples with 4 children each over 80 markers; a child is kept (affected) when it carries A2 at the causal marker and one of its
    parents is het there -> (g, trios of the kept children)."""
    g, called, trios = M.pedigree(120, 0, 80, seed=seed)
    rng = np.random.default_rng(seed + 1)
    cols, rows = [g], []
    n = 120
    for k in range(60):
        f, m = k, 60 + k
        for _ in range(4):
            hap = []
            for p in (f, m):
                a = np.where(g[:, p] == 0, rng.integers(0, 2, 80), (g[:, p] + 1) // 2)      # the allele passed: a het passes either
                hap.append(a)
            child = (hap[0] + hap[1] - 1).astype(np.int8)
            if child[causal] >= 0 and (g[causal, f] == 0 or g[causal, m] == 0):
                cols.append(child[:, None])
                rows.append((n, f, m))
                n += 1
    return np.concatenate(cols, axis=1), np.asarray(rows, dtype=np.int32)


def test_ascertained_children_point_at_the_planted_marker():
    """A sanity check of the whole chain on the host, not a power claim: the seed is chosen so that it holds."""
    from eagleeverything_amd import r_api
    g, trios = ascertained(seed=1)
    assert trios.shape[0] > 40
    s = r_api.tdt_summary(r_api.tdt_host(g, None, trios, seed=1, R=200))
    assert int(np.nanargmax(s["chisq"])) == 17 and s["T"][17] > s["U"][17]
    assert s["emp2"][17] == np.nanmin(s["emp2"]) and s["emp2"][17] < 0.05 and s["emp1"][17] <= s["emp2"][17]
    assert (s["emp1"][np.isfinite(s["emp1"])] <= s["emp2"][np.isfinite(s["emp2"])]).all()


def test_argument_rule_of_the_restatement():
    from eagleeverything_amd import r_api
    g = np.zeros((5, 4), dtype=np.int8)
    for kw in (dict(R=-1), dict(R=1.5), dict(R=1, first=0), dict(R=2, first=(1 << 31) - 1), dict(R=1, family=[0, 1]), dict(R=1, family=[65536]),
               dict(R=1, family=[-1]), dict(R=1, family=[0.5])):
        with pytest.raises(ValueError):
            r_api.tdt_host(g, None, [(2, 0, 1)], **kw)
    for trios in ([], [(0, 0, 1)], [(4, 0, 1)], [(2, 1, 1)]):
        with pytest.raises(ValueError):
            r_api.tdt_host(g, None, trios)
    ok = r_api.tdt_host(g, None, [(2, 0, 1)], R=1, first=(1 << 31) - 1, family=[65535])
    assert ok["trio"].tolist() == [[5, 5, 5, 5, 5, 5]] and ok["marker"].tolist() == [[0, 0, 0, 0, 1]] * 5
    assert [len(list(itertools.product(M.CODES, repeat=3))), len(M.error_triples())] == [64, 16]
