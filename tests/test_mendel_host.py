"""CPU: r_api.mendel_host and r_api.parentage_host -- the numpy restatements that the GPU tests compare the device with -- against the
plain loops over allele sets of tests/mendel_truth.py (include/eagle_hip.h section 1b'''viii), on simulated pedigrees with planted
errors, and the .fam readers.  Everything is integers: every comparison is ==."""
import itertools

import numpy as np
import pytest

import mendel_truth as T


def planted(founders, children, L, seed, miss):
    """A pedigree with every error triple planted into some recorded trio at some marker -> (g, called, trios, planted markers)."""
    g, called, trios = T.pedigree(founders, children, L, seed, miss)
    rng = np.random.default_rng(seed + 1)
    where = []
    for k, triple in enumerate(T.error_triples()):
        t, x = trios[k % trios.shape[0]], int(rng.integers(0, L))
        T.plant(g, called, t, x, triple)
        where.append(x)
    return g, called, trios, where


def test_exactly_sixteen_of_the_64_code_triples_are_errors():
    from eagleeverything_amd import r_api
    triples = list(itertools.product(T.CODES, repeat=3))
    errs = T.error_triples()
    assert len(triples) == 64 and len(errs) == 16
    g, called = np.zeros((64, 3), dtype=np.int8), np.zeros((64, 3), dtype=bool)
    for x, t in enumerate(triples):
        T.plant(g, called, (0, 1, 2), x, t)
    tab, marker = r_api.mendel_host(g, called, [[0, 1, 2]])
    assert tab[0, 5] == 16 and marker.sum() == 16 and marker.dtype == np.int32 and tab.dtype == np.int32
    assert [triples[x] for x in np.flatnonzero(marker)] == errs
    want, wmark = T.mendel_loops(g, called, [(0, 1, 2)])
    assert np.array_equal(tab, want) and np.array_equal(marker, wmark)
    # the counts of rule 4 on the same trio: 48 markers with the child called, 3/4 of them with a parent called
    assert tab[0].tolist() == [36, 8, 36, 8, 27, 16]
    # on the image every not-called entry is a het: other errors (a het child of two equal homozygotes appears, hidden parents' go)
    tab2, marker2 = r_api.mendel_host(g, None, [[0, 1, 2]])
    want2 = T.mendel_loops(g, None, [(0, 1, 2)])
    assert np.array_equal(tab2, want2[0]) and np.array_equal(marker2, want2[1]) and tab2[0, 4] == 64 and not np.array_equal(marker, marker2)


@pytest.mark.parametrize("miss", (0.0, 0.1))
def test_mendel_host_equals_the_loops_on_planted_pedigrees(miss):
    from eagleeverything_amd import r_api
    g, called, trios, where = planted(6, 14, 150, seed=5, miss=miss)
    lst = np.concatenate((trios, trios[:3], [[trios[0, 0], -1, trios[0, 2]], [trios[1, 0], trios[1, 1], -1], [trios[2, 0], -1, -1]])).astype(np.int32)
    assert np.isin(lst[:, 0], lst[:, 1:]).any()          # a child of one trio is a parent in another
    for cm in (called, None):
        tab, marker = r_api.mendel_host(g, cm, lst)
        want, wmark = T.mendel_loops(g, cm, lst.tolist())
        assert np.array_equal(tab, want) and np.array_equal(marker, wmark)
        assert tab[-1].tolist()[1:] == [0, 0, 0, 0, 0] and tab[-1, 0] == 0                # both parents unknown: nothing
        assert marker.sum() == tab[:, 5].sum() and tab[:, 5].sum() >= 10
    if miss == 0.0:
        assert all(marker[x] >= 1 for x, t in zip(where, T.error_triples()) if 3 not in t)
    with pytest.raises(ValueError):
        r_api.mendel_host(g, called, [[0, 0, 1]])
    with pytest.raises(ValueError):
        r_api.mendel_host(g, called, [[0, 1, 1]])
    with pytest.raises(ValueError):
        r_api.mendel_host(g, called, [[0, 1, g.shape[1]]])


@pytest.mark.parametrize("miss", (0.0, 0.15))
def test_parentage_host_equals_the_loops(miss):
    from eagleeverything_amd import r_api
    g, called, trios, _ = planted(8, 10, 120, seed=9, miss=miss)
    n = g.shape[1]
    off = trios[[0, 3, 9], 0]
    everybody = np.arange(n)
    cases = [(everybody[::2], everybody[1::2], 1, False), (everybody, everybody, 1, False), (everybody, everybody, 1, True),
             (everybody[:5], None, 1, False), (None, everybody[3:], 1, False), (everybody, everybody[::-1], 100, False),
             ([trios[0, 1]], [trios[0, 2]], 1, False), ([trios[0, 1]], None, 1, False)]
    for s, d, mo, selfing in cases:
        for cm in (called, None):
            got = r_api.parentage_host(g, cm, off, s, d, mo, selfing)
            want = T.parentage_loops(g, cm, off.tolist(), s, d, mo, selfing)
            assert got.dtype == np.int32 and np.array_equal(got, want), (s, d, mo, selfing)
    assert (r_api.parentage_host(g, called, off, [trios[0, 1]], [trios[0, 2]])[:, 1] == -1).all()   # one candidate: no runner-up
    for bad in (dict(offspring=[]), dict(sires=None, dams=None), dict(sires=[1, 1]), dict(offspring=[2, 2]), dict(dams=[n]), dict(sires=[-1]),
                dict(min_overlap=-1), dict(allow_self=2)):
        kw = dict(offspring=off, sires=[0, 1], dams=[4, 5], min_overlap=1, allow_self=False)
        kw.update(bad)
        with pytest.raises(ValueError):
            r_api.parentage_host(g, called, **kw)


def test_true_parents_of_an_error_free_pedigree_are_assigned():
    from eagleeverything_amd import r_api
    g, called, trios = T.pedigree(10, 12, 400, seed=21)
    n = g.shape[1]
    tab, marker = r_api.mendel_host(g, called, trios)
    assert not tab[:, 5].any() and not marker.any() and (tab[:, [0, 2, 4]] == 400).all()
    everybody = np.arange(n)
    best = r_api.parentage_host(g, None, trios[:, 0], everybody, everybody)
    res = r_api.parentage_summary(trios[:, 0], best)
    assert (res["errors"] == 0).all() and res["assigned"].all() and (res["overlap"] == 400).all()
    # sire and dam are positions in the search, not sexes: the true pair comes back in the order of the smaller ordinal
    assert np.array_equal(np.sort(best[:, 0, :2], axis=1), np.sort(trios[:, 1:], axis=1))
    assert np.array_equal(best[:, 1, :2], best[:, 0, 1::-1]) and (res["gap"] == 0).all()     # the runner-up is the same pair, swapped
    for c, f, m in trios[:4].tolist():                   # with each true parent in one list alone, nobody else fits 400 markers
        res = r_api.parentage_summary([c], r_api.parentage_host(g, None, [c], everybody[everybody != m], everybody[everybody != f]))
        assert (res["sire"][0], res["dam"][0], res["errors"][0]) == (f, m, 0) and res["gap"][0] > 0 and res["assigned"][0]
    # single-parent assignment finds a true parent too
    one = r_api.parentage_host(g, None, trios[:, 0], everybody, None)
    assert (one[:, 0, 2] == 0).all() and (one[:, 0, 1] == -1).all() and all(s in t[1:] for s, t in zip(one[:, 0, 0], trios))


def test_ties_go_to_the_smaller_ordinal_and_the_filters_exclude():
    from eagleeverything_amd import r_api
    g, called, trios = T.pedigree(6, 4, 300, seed=33, miss=0.2)
    c, f, m = trios[0].tolist()
    n = g.shape[1]
    g = np.concatenate((g, g[:, [f]]), axis=1)            # individual n is a copy of the father
    called = np.concatenate((called, called[:, [f]]), axis=1)
    for sires in ([n, f], [f, n]):
        best = r_api.parentage_host(g, called, [c], sires, [m])
        assert best[0, 0, 0] == sires[0] and best[0, 1, 0] == sires[1] and best[0, 0, 2] == best[0, 1, 2] == 0
        assert np.array_equal(best[0, 0, 2:], best[0, 1, 2:])
    # min_overlap: the true father's overlap is what bed_parentage would count; one more cuts him out
    ov = int(np.count_nonzero(called[:, c] & called[:, f] & called[:, m]))
    others = [i for i in range(6) if i not in (f, m)]
    assert r_api.parentage_host(g, called, [c], [f] + others, [m], ov)[0, 0, 0] == f
    cut = r_api.parentage_host(g, called, [c], [f] + others, [m], ov + 1)
    assert f not in cut[0, :, 0] and (cut[0, :, 3][cut[0, :, 3] >= 0] > ov).all()
    assert np.array_equal(cut, T.parentage_loops(g, called, [c], [f] + others, [m], ov + 1))
    # the offspring itself is in both lists and never its own parent; selfing only when allowed
    lst = [c, f, m]
    a = r_api.parentage_host(g, called, [c], lst, lst, 1, False)
    b = r_api.parentage_host(g, called, [c], lst, lst, 1, True)
    assert c not in a[0, :, :2] and c not in b[0, :, :2]
    assert all(r[0] != r[1] for r in a[0].tolist()) and np.array_equal(b, T.parentage_loops(g, called, [c], lst, lst, 1, True))
    cands = lambda selfing: sum(1 for s in lst for d in lst if s != c and d != c and (selfing or s != d))
    assert cands(False) == 2 and cands(True) == 4


def test_summaries_and_the_marker_mask():
    from eagleeverything_amd import r_api
    g, called, trios, _ = planted(6, 8, 100, seed=2, miss=0.0)
    lst = np.concatenate((trios, [[trios[0, 0], -1, trios[0, 2]]])).astype(np.int32)
    tab, marker = r_api.mendel_host(g, called, lst)
    res = r_api.mendel_summary(lst, tab, marker, g.shape[1])
    assert np.array_equal(res["errors"], tab[:, 5]) and res["errors_as_child"].sum() == tab[:, 5].sum()
    assert res["errors_as_parent"].sum() == sum(int(e) * int((t[1:] >= 0).sum()) for t, e in zip(lst, tab[:, 5]))
    assert np.array_equal(res["rate"], tab[:, 5] / (tab[:, 0] + tab[:, 2] - tab[:, 4]).astype(np.float64))
    assert np.array_equal(res["marker_rate"], marker / np.float64(lst.shape[0]))
    keep = r_api.mendel_keep_mask(marker, lst.shape[0], 0.2)
    assert keep.dtype == bool and np.array_equal(keep, marker <= 1) and not keep.all() and keep.any()
    assert r_api.mendel_keep_mask(marker, lst.shape[0], 1.0).all()
    with pytest.raises(ValueError):
        r_api.mendel_keep_mask(marker, 0, 0.1)
    with pytest.raises(ValueError):
        r_api.mendel_keep_mask(marker, 1, 0.1)             # more errors than trios


def test_ReadFam_and_fam_trios(tmp_path):
    from eagleeverything_amd import r_api
    fam = tmp_path / "p.fam"
    fam.write_text("F1 a 0 0 1 -9\nF1 b 0 0 2 -9\nF1 c a b 1 1.5\nF1 d a 0 2 -9\nF1 e zz b 0 -9\nF1 f zz 0 0 -9\n\nF2 a 0 0 1 -9\nF2 c a b 2 -9\n")
    d = r_api.ReadFam(str(fam))
    assert list(d) == ["FID", "IID", "Father", "Mother", "Sex", "Pheno"] and d["IID"] == ["a", "b", "c", "d", "e", "f", "a", "c"]
    assert d["Father"][2] == "a" and d["Mother"][2] == "b" and d["Sex"][1] == "2" and d["Pheno"][2] == "1.5" and d["FID"][6] == "F2"
    tr = r_api.fam_trios(d)
    # parents are looked up inside the family: F2's c has father F2 a (index 6) and no mother b in F2
    assert tr.dtype == np.int32 and tr.tolist() == [[2, 0, 1], [3, 0, -1], [4, -1, 1], [7, 6, -1]]
    assert np.array_equal(r_api.fam_trios(str(fam)), tr)
    (tmp_path / "short.fam").write_text("F1 a 0 0 1\n")
    with pytest.raises(ValueError):
        r_api.ReadFam(str(tmp_path / "short.fam"))
    for text in ("F1 a 0 0 1 -9\nF1 a 0 0 1 -9\n", "F1 a a 0 1 -9\n", "F1 a 0 0 1 -9\nF1 b a a 1 -9\n"):
        (tmp_path / "bad.fam").write_text(text)
        with pytest.raises(ValueError):
            r_api.fam_trios(str(tmp_path / "bad.fam"))
    (tmp_path / "none.fam").write_text("F1 a 0 0 1 -9\n")
    assert r_api.fam_trios(str(tmp_path / "none.fam")).shape == (0, 3)
