"""Mendel errors and parentage assignment on the GPU from the ingested panel: eagle_mendel (k_ibd_planes_i8, k_mendel_trios) and
eagle_parentage (k_plane_gather, k_parentage, k_parentage_finish) on M.ascii.

The device's tables are compared with r_api.mendel_host / r_api.parentage_host -- the numpy restatements that tests/test_mendel_host.py
pins to plain loops over allele sets (include/eagle_hip.h section 1b'''viii).  Everything is integers: every comparison is ==."""
import functools

import numpy as np
import pytest

import mendel_truth as T
from test_gpu_ibd import write_M

pytestmark = pytest.mark.gpu

NS = (3, 64, 65, 129)                                    # one trio of individuals, and the edges of the 64-individual plane groups
LS = (1, 63, 64, 65, 129, 1000)                          # a short last word, a full one, one marker past it
TS = (1, 63, 64, 65, 130)                                # the edges of the 64-trio waves
N_O = (1, 5)
N_S = (1, 3, 64, 65)                                     # one sire, a partial group of four, the edges of a 16-sire workgroup's last wave
N_D = (0, 1, 63, 64, 65, 130)                            # the unknown dam, and the edges of the 64-dam tiles


def trio_list(n, count, seed):
    """`count` trios over n individuals: the first six are a full trio, its father unknown, its mother unknown, both unknown, the full
    trio again, and a trio in which the first one's father is the child; then valid trios at random (a fifth with an unknown parent)."""
    rng = np.random.default_rng(seed)
    out = [(2, 0, 1), (2, -1, 1), (2, 0, -1), (2, -1, -1), (2, 0, 1), (0, 1, 2)]
    while len(out) < count:
        c, f, m = rng.choice(n, 3, replace=False).tolist()
        u = rng.random()
        out.append((c, -1 if u < 0.1 else f, -1 if 0.1 <= u < 0.2 else m))
    return np.asarray(out[:count], dtype=np.int32)


def edge_markers(L):
    """Bits 0 and 63 of every word, and the last marker."""
    return sorted({x for x in range(L) if x % 64 in (0, 63)} | {L - 1})


def random_panel(n, L, seed, miss=0.0):
    """Genotypes at random (every trio has errors) with the 16 error triples cycled through the edge markers of the trio (2, 0, 1)."""
    rng = np.random.default_rng(seed)
    g = rng.integers(-1, 2, (L, n)).astype(np.int8)
    called = rng.random((L, n)) >= miss if miss > 0 else np.ones((L, n), dtype=bool)
    kinds = T.error_triples()
    for k, x in enumerate(edge_markers(L)):
        T.plant(g, called, (2, 0, 1), x, kinds[(k + seed) % 16])
    g[~called] = 0
    return g, called


@functools.lru_cache(maxsize=None)
def kinds_panel(L, hide):
    """48 individuals in 16 trios (3 k + 2, 3 k, 3 k + 1) of an error-free pedigree; trio k gets error triple k at every edge marker.
    hide: the not-called codes of the triples stay not called (the .bed route); else they are hets (the image) -> (g, called, trios)."""
    rng = np.random.default_rng(L)
    g, called = np.zeros((L, 64), dtype=np.int8), np.ones((L, 64), dtype=bool)
    trios = np.asarray([(3 * k + 2, 3 * k, 3 * k + 1) for k in range(16)], dtype=np.int32)
    g[:, 48:] = rng.integers(-1, 2, (L, 16))
    for k, (c, f, m) in enumerate(trios.tolist()):
        hap = rng.integers(0, 2, (4, L))
        g[:, f], g[:, m] = hap[0] + hap[1] - 1, hap[2] + hap[3] - 1
        pick = rng.integers(0, 2, (2, L))
        g[:, c] = np.where(pick[0], hap[0], hap[1]) + np.where(pick[1], hap[2], hap[3]) - 1
        for x in edge_markers(L):
            T.plant(g, called, (c, f, m), x, T.error_triples()[k])
    if not hide:
        called[:] = True
    for a in (g, called, trios):
        a.setflags(write=False)
    return g, called, trios


def same_rows(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist(), got[got != want][:5], want[got != want][:5])


@pytest.mark.parametrize("n", NS)
def test_gpu_mendel_equals_host_at_word_and_wave_edges(tmp_path, n):
    from eagleeverything_amd import r_api, rcpp_api
    rcpp_api.drop_cache()
    errors = 0
    for L in LS:
        g, _ = random_panel(n, L, seed=100 * n + L)
        g[L - 1, [2, 0, 1]] = (0, -1, -1)                # a het child of two hom A1 parents on the last marker: an error on the image
        M = write_M(tmp_path, g, "M%d.ascii" % L)
        for count in TS:
            trios = trio_list(n, count, seed=n + L + count)
            want_tab, want_marker = r_api.mendel_host(g, None, trios)
            tab, marker = rcpp_api.mendel(M, (n, L), trios)
            same_rows(tab, want_tab, (n, L, count, "trio"))
            same_rows(marker, want_marker, (n, L, count, "marker"))
            assert marker[L - 1] >= 1 and marker.sum() == tab[:, 5].sum()
            assert (tab[trios[:, 1] >= 0, 0] == L).all() and (tab[trios[:, 1] < 0, 0] == 0).all()          # n_cf = L or 0 on the image
            assert (tab[(trios[:, 1:] >= 0).all(axis=1), 4] == L).all() and (tab[(trios[:, 1:] < 0).any(axis=1), 4] == 0).all()
            if count >= 6:
                assert tab[3].tolist() == [0, 0, 0, 0, 0, 0] and np.array_equal(tab[0], tab[4])            # both unknown; the repeated trio
                assert tab[1, 5] == tab[1, 3] and tab[2, 5] == tab[2, 1]                                    # one parent: its opposite homozygotes
            errors += int(tab[:, 5].sum())
        only, none = rcpp_api.mendel(M, (n, L), trios, markers=False)
        assert none is None
        same_rows(only, want_tab, (n, L, "without the marker counts"))
    assert errors > 0
    rcpp_api.drop_cache()


@pytest.mark.parametrize("L", (65, 129, 1000))
def test_gpu_mendel_every_error_kind_at_bits_0_and_63_and_the_last_marker(tmp_path, L):
    from eagleeverything_amd import r_api, rcpp_api
    g, _, trios = kinds_panel(L, False)
    rcpp_api.drop_cache()
    M = write_M(tmp_path, g)
    want_tab, want_marker = r_api.mendel_host(g, None, trios)
    tab, marker = rcpp_api.mendel(M, (64, L), trios)
    same_rows(tab, want_tab, "trio")
    same_rows(marker, want_marker, "marker")
    edges = edge_markers(L)
    assert L % 64 != 0 and L - 1 in edges and (marker[edges] >= 1).all()
    # on the image a not-called code is a het: the 16 triples are those of three called codes that are errors
    as_het = [tuple(1 if c == 3 else c for c in t) for t in T.error_triples()]
    is_err = [T.is_error(T.G_OF_CODE[c], True, T.G_OF_CODE[f], True, T.G_OF_CODE[m], True) for c, f, m in as_het]
    assert (marker[edges] == sum(is_err)).all() and [int(e >= len(edges)) for e in tab[:, 5]] == [int(b) for b in is_err]
    if L == 65:
        loops = T.mendel_loops(g, None, trios.tolist())
        assert np.array_equal(tab, loops[0]) and np.array_equal(marker, loops[1])
    rcpp_api.drop_cache()


@functools.lru_cache(maxsize=None)
def assignment_panel(miss):
    """150 founders and 60 children over 300 markers, then individual 210 = a copy of the first child's father -> (g, called, trios)."""
    g, called, trios = T.pedigree(150, 60, 300, seed=4, miss=miss)
    f = int(trios[0, 1])
    g, called = np.concatenate((g, g[:, [f]]), axis=1), np.concatenate((called, called[:, [f]]), axis=1)
    for a in (g, called, trios):
        a.setflags(write=False)
    return g, called, trios


def candidate_lists(n, trios, n_o, n_s, n_d, seed):
    """Offspring = the first n_o children.  The sire list starts with the first child's father, the child itself and the child's mother;
    the dam list with the mother, the child and the father: the offspring is in both lists, and so are its parents."""
    rng = np.random.default_rng(seed)
    c, f, m = trios[0].tolist()
    rest = [i for i in rng.permutation(n).tolist() if i not in (c, f, m)]
    return trios[:n_o, 0].copy(), np.asarray([f, c, m] + rest, dtype=np.int32)[:n_s], np.asarray([m, c, f] + rest[::-1], dtype=np.int32)[:n_d]


@pytest.mark.parametrize("n_o", N_O)
def test_gpu_parentage_equals_host_at_tile_edges(tmp_path, n_o):
    from eagleeverything_amd import r_api, rcpp_api
    g, _, trios = assignment_panel(0.0)
    L, n = g.shape
    rcpp_api.drop_cache()
    M = write_M(tmp_path, g)
    for n_s in N_S + (0,):
        for n_d in N_D:
            if n_s == 0 and n_d == 0:
                continue
            off, sires, dams = candidate_lists(n, trios, n_o, n_s, n_d, seed=n_s + n_d)
            for selfing in (False, True):
                want = r_api.parentage_host(g, None, off, sires, dams, 1, selfing)
                got = rcpp_api.parentage(M, (n, L), off, sires, dams, 1, selfing)
                same_rows(got, want, (n_o, n_s, n_d, selfing))
                assert off[0] not in got[0, :, :2]                       # never its own parent
                if n_s >= 3 and n_d >= 3:                                # the parents are in both lists: (f, m) and (m, f), no error
                    assert got[0, 0].tolist() == [trios[0, 1], trios[0, 2], 0, L] and got[0, 1].tolist() == [trios[0, 2], trios[0, 1], 0, L]
                    if not selfing:
                        assert (got[:, :, 0] != got[:, :, 1]).all()
                if n_s * n_d == 1 or (n_s, n_d) in ((1, 0), (0, 1)):     # one candidate: no runner-up
                    assert (got[:, 1] == -1).all() and got[0, 0, 2] == 0
    rcpp_api.drop_cache()


def test_gpu_parentage_true_parents_ties_self_and_too_few_candidates(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    g, _, trios = assignment_panel(0.0)
    L, n = g.shape
    rcpp_api.drop_cache()
    M = write_M(tmp_path, g)
    # the true parents of every child, each in one list alone, come back with e = 0
    sires = np.setdiff1d(np.arange(n - 1), trios[:, 2])
    dams = np.setdiff1d(np.arange(n - 1), trios[:, 1])
    got = rcpp_api.parentage(M, (n, L), trios[:, 0], sires, dams)
    same_rows(got, r_api.parentage_host(g, None, trios[:, 0], sires, dams), "every child")
    assert np.array_equal(got[:, 0, :2], trios[:, 1:]) and (got[:, 0, 2] == 0).all() and (got[:, 1, 2] > 0).all()
    res = r_api.parentage_summary(trios[:, 0], got)
    assert res["assigned"].all() and (res["gap"] > 0).all()
    # a duplicated genotype ties and the earlier candidate wins, whichever comes first
    c, f, m = trios[0].tolist()
    for pair in ([n - 1, f], [f, n - 1]):
        lst = np.asarray(pair + [3, 4, 5], dtype=np.int32)
        got = rcpp_api.parentage(M, (n, L), [c], lst, [m])
        assert got[0, :, 0].tolist() == pair and got[0, :, 2].tolist() == [0, 0] and got[0, :, 1].tolist() == [m, m]
        single = rcpp_api.parentage(M, (n, L), [c], lst, None)
        assert single[0, :, 0].tolist() == pair and (single[0, :, 1] == -1).all() and single[0, :, 2].tolist() == [0, 0]
        same_rows(single, r_api.parentage_host(g, None, [c], lst, None), "single parent")
    # one individual in both lists: a candidate only with allow_self
    both = np.asarray([f], dtype=np.int32)
    assert (rcpp_api.parentage(M, (n, L), [c], both, both) == -1).all()
    got = rcpp_api.parentage(M, (n, L), [c], both, both, allow_self=True)
    assert got[0, 0, :2].tolist() == [f, f] and got[0, 0, 3] == L and (got[0, 1] == -1).all()
    same_rows(got, r_api.parentage_host(g, None, [c], both, both, 1, True), "selfing")
    # no admissible candidate at all: the offspring is the only sire; min_overlap above L
    assert (rcpp_api.parentage(M, (n, L), [c], [c], None) == -1).all()
    assert (rcpp_api.parentage(M, (n, L), [c], [f], [m], min_overlap=L + 1) == -1).all()
    assert rcpp_api.parentage(M, (n, L), [c], [f], [m], min_overlap=L)[0, 0].tolist() == [f, m, 0, L]
    rcpp_api.drop_cache()


def test_gpu_mendel_and_parentage_streamed_equal_resident(tmp_path, monkeypatch):
    """700 individuals x 2,100 markers is 1.8 MB of image: under a budget of 1 MB it goes in bands of whole lines, and the planes still fit."""
    from eagleeverything_amd import _lib, r_api, rcpp_api
    g, _, trios = T.pedigree(400, 300, 2100, seed=6)
    L, n = g.shape
    rng = np.random.default_rng(1)
    wrong = trios.copy()
    wrong[::7, 1] = rng.permutation(200)[:wrong[::7].shape[0]]                  # sire founders as recorded fathers: errors; never the child or the mother
    lst = np.concatenate((trios, wrong, [[255, 256, 699], [699, 0, 255], [256, -1, 511]])).astype(np.int32)   # across the bands of 256 lines
    off, sires, dams = trios[::40, 0].copy(), np.arange(0, 400, 3, dtype=np.int32), np.arange(1, 700, 5, dtype=np.int32)
    M = write_M(tmp_path, g)
    rcpp_api.drop_cache()
    tab, marker = rcpp_api.mendel(M, (n, L), lst)
    best = rcpp_api.parentage(M, (n, L), off, sires, dams)
    want = r_api.mendel_host(g, None, lst)
    same_rows(tab, want[0], "resident trio")
    same_rows(marker, want[1], "resident marker")
    same_rows(best, r_api.parentage_host(g, None, off, sires, dams), "resident parentage")
    assert tab[:300, 5].sum() == 0 and tab[300:600, 5].sum() > 0
    rcpp_api.drop_cache()
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.001")
    tab2, marker2 = rcpp_api.mendel(M, (n, L), lst)
    assert tab2.tobytes() == tab.tobytes() and marker2.tobytes() == marker.tobytes()
    assert rcpp_api.parentage(M, (n, L), off, sires, dams).tobytes() == best.tobytes()
    # a budget the planes do not fit: refused before any kernel runs
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.0001")
    for call in (lambda: rcpp_api.mendel(M, (n, L), lst), lambda: rcpp_api.parentage(M, (n, L), off, sires, dams)):
        with pytest.raises(_lib.EagleError) as err:
            call()
        assert err.value.code == -4 and "do not fit the memory budget" in err.value.text
    rcpp_api.drop_cache()


def test_gpu_mendel_and_parentage_view_alias_gives_the_kept_individuals(tmp_path):
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    g, _, trios = T.pedigree(40, 30, 300, seed=12)
    L, n = g.shape
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), g)
    drop = np.array([1, 2, 33, 64, 65, 70])              # 1-based, as AM's indxNA
    kept = np.setdiff1d(np.arange(n), drop - 1)
    sub = am.reshape_geno(geno, drop, view=True)
    nk = n - drop.size
    assert list(sub["dim_of_ascii_M"]) == [nk, L]
    new = np.full(n, -1)
    new[kept] = np.arange(nk)
    lst = new[trios]                                     # a dropped parent is an unknown one; a dropped child leaves
    lst = np.ascontiguousarray(lst[lst[:, 0] >= 0], dtype=np.int32)
    assert (lst[:, 1:] < 0).any() and lst.shape[0] > 20
    tab, marker = rcpp_api.mendel(sub["asciifileM"], (nk, L), lst)
    want = r_api.mendel_host(g[:, kept], None, lst)
    same_rows(tab, want[0], "view trio")
    same_rows(marker, want[1], "view marker")
    everybody = np.arange(nk, dtype=np.int32)
    best = rcpp_api.parentage(sub["asciifileM"], (nk, L), lst[:5, 0], everybody, everybody)
    same_rows(best, r_api.parentage_host(g[:, kept], None, lst[:5, 0], everybody, everybody), "view parentage")
    rcpp_api.drop_cache()
