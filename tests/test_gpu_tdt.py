"""The transmission disequilibrium test on the GPU from the ingested panel: eagle_tdt (k_ibd_planes_i8, then k_tdt_trios, k_tdt_finish and,
with flips, k_tdt_image, k_tdt_signs and the max(T) tile and finish of eagle_maxt.hip) on M.ascii.

The device's words are compared with r_api.tdt_host -- the numpy restatement that tests/test_tdt_host.py pins to plain loops over allele
choices (include/eagle_hip.h section 1b''''viii).  Integers, and two correctly rounded fp64 operations on exact operands: every
comparison is ==."""
import numpy as np
import pytest

import mendel_truth as M
import regimes_truth as R
import tdt_truth as T
from test_gpu_ibd import write_M
from test_gpu_mendel import LS, NS, TS, trio_list

pytestmark = pytest.mark.gpu

FLIP_TRIOS = (1, 15, 16, 17, 127, 128, 129, 257)         # the tile's 16-byte and 128-byte K edges
FLIP_LS = (1, 127, 128, 129, 300)                        # the edges of the 128-marker tiles
FLIP_RS = (1, 31, 32, 33, 128, 129)                      # the edges of the 32-flip blocks and of a workgroup's 128 flips


def sib_trios(founders, count, seed):
    """`count` trios over 2 * founders parents (father k, mother founders + k) with about three sibs a couple, one trio with an unknown
    mother among them, and the children numbered after the parents -> int32 (count, 3), the number of individuals."""
    rng = np.random.default_rng(seed)
    couple = rng.integers(0, founders, count)
    tr = np.stack([2 * founders + np.arange(count), couple, founders + couple], axis=1).astype(np.int32)
    if count > 2:
        tr[count // 2, 2] = -1
    return tr, 2 * founders + count


def sib_panel(founders, count, L, seed):
    """Random parents, every child drawn from its parents by Mendel's rule (a het passes either allele) -> (g int8 (L, n), trios)."""
    tr, n = sib_trios(founders, count, seed)
    rng = np.random.default_rng(seed + 1)
    g = np.zeros((L, n), dtype=np.int8)
    g[:, :2 * founders] = rng.integers(-1, 2, (L, 2 * founders))
    for c, f, m in tr.tolist():
        m = m if m >= 0 else founders                    # the unknown mother: drawn from somebody
        a = np.where(g[:, f] == 0, rng.integers(0, 2, L), (g[:, f] + 1) // 2)
        b = np.where(g[:, m] == 0, rng.integers(0, 2, L), (g[:, m] + 1) // 2)
        g[:, c] = a + b - 1
    return g, tr


@pytest.mark.parametrize("n", NS)
def test_gpu_tdt_counts_equal_host_at_word_and_wave_edges(tmp_path, n):
    from eagleeverything_amd import r_api, rcpp_api
    rcpp_api.drop_cache()
    informative = 0
    for L in LS:
        g = np.random.default_rng(100 * n + L).integers(-1, 2, (L, n)).astype(np.int8)
        g[L - 1, [2, 0, 1]] = (0, 0, -1)                 # a het father passes A2 to the het child of a hom A1 mother on the last marker
        Mf = write_M(tmp_path, g, "M%d.ascii" % L)
        for count in TS:
            trios = trio_list(n, count, seed=n + L + count)
            want = r_api.tdt_host(g, None, trios)
            got = rcpp_api.tdt(Mf, (n, L), trios)
            T.same(got, want, (n, L, count))
            assert got["marker"][L - 1, 0] >= 1 and got["maxkey"].size == 0 and not got["count1"].any()
            assert got["marker"][:, [0, 2, 4]].sum() == got["trio"][:, 3].sum() and got["marker"][:, 4].sum() == got["trio"][:, 5].sum()
            assert not got["trio"][(trios[:, 1:] < 0).any(axis=1)].any()                                       # an unknown parent: nothing
            if count >= 6:
                assert np.array_equal(got["trio"][0], got["trio"][4])                                          # the repeated trio
            informative += int(got["trio"][:, 1:3].sum())
    assert informative > 0
    rcpp_api.drop_cache()


@pytest.mark.parametrize("L", (65, 129, 1000))
def test_gpu_tdt_every_informative_and_error_kind_at_bits_0_and_63_and_the_last_marker(tmp_path, L):
    from eagleeverything_amd import r_api, rcpp_api
    g, _, trios = T.kinds_panel(L, False)
    rcpp_api.drop_cache()
    Mf = write_M(tmp_path, g)
    want = r_api.tdt_host(g, None, trios, seed=L, R=33)
    got = rcpp_api.tdt(Mf, (84, L), trios, seed=L, R=33)
    T.same(got, want, L)
    edges = T.edge_markers(L)
    table = T.triple_table()
    assert L % 64 != 0 and L - 1 in edges
    per_marker = np.sum([table[t][:5] for t in T.informative_triples()], axis=0)
    # on the image a not-called code of an error triple is a het, which may make the triple informative: the 11 are a lower bound
    assert (got["marker"][edges] >= per_marker).all() and (got["marker"][edges].sum(axis=1) >= 11).all()
    if L == 65:
        T.same(got, T.tdt_loops(g, None, trios, seed=L, R=33), "loops")
    rcpp_api.drop_cache()


@pytest.mark.parametrize("count", FLIP_TRIOS)
def test_gpu_tdt_flips_equal_host_at_tile_edges(tmp_path, count):
    from eagleeverything_amd import r_api, rcpp_api
    rcpp_api.drop_cache()
    reached = 0
    for L in FLIP_LS:
        g, trios = sib_panel(max(1, count // 3), count, L, seed=count + L)
        n = g.shape[1]
        Mf = write_M(tmp_path, g, "M%d.ascii" % L)
        for Rn in FLIP_RS:
            want = r_api.tdt_host(g, None, trios, seed=count, first=3, R=Rn)
            got = rcpp_api.tdt(Mf, (n, L), trios, seed=count, first=3, R=Rn)
            T.same(got, want, (count, L, Rn))
            assert got["maxkey"].shape == (Rn,) and (got["argmax"] < L).all() and (got["count1"] <= Rn).all()
            reached += int(got["count1"].sum())
        if count > 2:
            assert got["marker"].sum() > 0
    # explicit families: every trio its own, and all of them one (every flip is then +-d_obs)
    own = np.arange(count, dtype=np.int32) * (65535 // max(count - 1, 1))
    T.same(rcpp_api.tdt(Mf, (n, L), trios, own, 5, 1, 33), r_api.tdt_host(g, None, trios, own, 5, 1, 33), "own families")
    one = rcpp_api.tdt(Mf, (n, L), trios, np.full(count, 65535), 5, 1, 33)
    T.same(one, r_api.tdt_host(g, None, trios, np.full(count, 65535), 5, 1, 33), "one family")
    assert (one["count1"] == 33).all() and (one["maxkey"] == one["key_obs"].max()).all() and (one["argmax"] == one["key_obs"].argmax()).all()
    assert reached > 0
    rcpp_api.drop_cache()


def test_gpu_tdt_split_calls_add_and_more_than_1024_flips(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api
    g, trios = sib_panel(40, 129, 300, seed=8)
    n, L = g.shape[1], 300
    rcpp_api.drop_cache()
    Mf = write_M(tmp_path, g)
    whole = rcpp_api.tdt(Mf, (n, L), trios, seed=2, first=1, R=160)
    a, b = rcpp_api.tdt(Mf, (n, L), trios, seed=2, first=1, R=33), rcpp_api.tdt(Mf, (n, L), trios, seed=2, first=34, R=127)
    assert np.array_equal(a["count1"] + b["count1"], whole["count1"])
    assert np.array_equal(np.concatenate([a["maxkey"], b["maxkey"]]), whole["maxkey"])
    assert np.array_equal(np.concatenate([a["argmax"], b["argmax"]]), whole["argmax"])
    for k in ("trio", "marker", "key_obs"):
        assert np.array_equal(a[k], whole[k]) and np.array_equal(b[k], whole[k])
    # the wrapper loops calls of at most 1,024 flips
    many = rcpp_api.tdt(Mf, (n, L), trios, seed=2, first=1, R=1100)
    T.same(many, r_api.tdt_host(g, None, trios, seed=2, first=1, R=1100), "1,100 flips")
    assert np.array_equal(many["maxkey"][:160], whole["maxkey"])
    rcpp_api.drop_cache()


def test_gpu_tdt_streamed_and_banded_equal_resident(tmp_path, monkeypatch):
    """700 individuals x 2,100 markers is 1.8 MB of image: under a budget of 0.7 MB it goes in bands of whole lines, and the planes (372 KB)
    still fit with the arrays of the call (139 KB); the image of d, 2,176 x 272 = 592 KB, then does not fit beside them and is built and
    multiplied in four bands of 640 markers."""
    from eagleeverything_amd import _lib, r_api, rcpp_api
    g, _, trios = M.pedigree(400, 300, 2100, seed=6)
    L, n = g.shape
    rng = np.random.default_rng(1)
    wrong = trios.copy()
    wrong[::7, 1] = rng.permutation(200)[:wrong[::7].shape[0]]                  # sire founders as recorded fathers: Mendel errors
    lst = np.concatenate((trios[:200], wrong[:54], [[255, 256, 699], [699, 0, 255], [256, -1, 511]])).astype(np.int32)   # across the bands of 256 lines
    assert lst.shape[0] == 257
    Mf = write_M(tmp_path, g)
    rcpp_api.drop_cache()
    want = r_api.tdt_host(g, None, lst, seed=4, R=40)
    res = rcpp_api.tdt(Mf, (n, L), lst, seed=4, R=40)
    T.same(res, want, "resident")
    assert res["trio"][:200, 0].min() == L and res["trio"][200:254, 0].min() < L                 # the wrong fathers cost complete markers
    rcpp_api.drop_cache()
    planes = 2 * ((L + 63) // 64) * ((n + 63) // 64 * 64) * 8
    fixed = 36 * 257 + 44 * L + 4 * 257 + 8 * L + 40 * 272 + 12 * 40 * ((L + 127) // 128) + 12 * 40
    image = ((L + 127) // 128 * 128) * 272
    assert planes + fixed + 3 * 128 * 272 < 700000 < planes + fixed + image
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.0007")
    banded = rcpp_api.tdt(Mf, (n, L), lst, seed=4, R=40)
    T.same(banded, want, "streamed and banded")
    # a budget that one band of 128 markers does not fit beside the planes, then one the planes do not fit: refused before any kernel runs
    for gb in (repr((planes + fixed + 100) / 1e9), "0.0001"):
        monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", gb)
        with pytest.raises(_lib.EagleError) as err:
            rcpp_api.tdt(Mf, (n, L), lst, seed=4, R=40)
        assert err.value.code == -4 and "do not fit the memory budget" in err.value.text and "the image band" in err.value.text
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", repr((planes + fixed + 100) / 1e9))
    T.same(rcpp_api.tdt(Mf, (n, L), lst), r_api.tdt_host(g, None, lst), "counts only need no image")
    rcpp_api.drop_cache()


def test_gpu_tdt_view_alias_gives_the_kept_individuals(tmp_path):
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    g, _, trios = M.pedigree(40, 30, 300, seed=12)
    L, n = g.shape
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), g)
    drop = np.array([1, 2, 33, 64, 65, 70])              # 1-based, as AM's indxNA
    kept = np.setdiff1d(np.arange(n), drop - 1)
    sub = am.reshape_geno(geno, drop, view=True)
    nk = n - drop.size
    new = np.full(n, -1)
    new[kept] = np.arange(nk)
    lst = new[trios]                                     # a dropped parent is an unknown one; a dropped child leaves
    lst = np.ascontiguousarray(lst[lst[:, 0] >= 0], dtype=np.int32)
    assert (lst[:, 1:] < 0).any() and lst.shape[0] > 20
    got = rcpp_api.tdt(sub["asciifileM"], (nk, L), lst, seed=1, R=17)
    T.same(got, r_api.tdt_host(g[:, kept], None, lst, seed=1, R=17), "view")
    assert got["marker"].sum() > 0
    rcpp_api.drop_cache()


def test_gpu_TDT_end_to_end_with_affected_children(tmp_path):
    from eagleeverything_amd import r_api, rcpp_api, synth
    g, trios = sib_panel(20, 60, 200, seed=3)
    n, L = g.shape[1], 200
    rcpp_api.drop_cache()
    geno = synth.write_geno_pair(str(tmp_path), g)
    affected = np.zeros(n, dtype=bool)
    affected[trios[::2, 0]] = True
    res = r_api.TDT(geno, trios=trios, affected=affected, R=50, seed=6)
    used = trios[::2]
    ref = r_api.tdt_summary(r_api.tdt_host(g, None, used, seed=6, R=50))
    assert np.array_equal(res["trios"], used) and sorted(res) == sorted(list(ref) + ["trios"])
    for k in ref:
        assert np.array_equal(res[k], ref[k], equal_nan=True), k
    everybody = r_api.TDT(geno, trios=trios)
    assert everybody["R"] == 0 and "emp1" not in everybody and np.array_equal(everybody["marker"], r_api.tdt_host(g, None, trios)["marker"])
    more = r_api.tdt_merge(res, r_api.TDT(geno, trios=trios, affected=affected, R=30, seed=6, first=51))
    assert np.array_equal(more["count1"], r_api.tdt_host(g, None, used, seed=6, R=80)["count1"]) and more["R"] == 80
    with pytest.raises(ValueError):
        r_api.TDT(geno, trios=trios, affected=np.zeros(n, dtype=bool))
    with pytest.raises(ValueError):
        r_api.TDT(geno)                                  # no trios, no fam, no bed
    rcpp_api.drop_cache()


def test_gpu_tdt_past_65535_plane_words(tmp_path):
    """One trio of three individuals over 64 x 65,535 + 65 markers: 65,537 plane words, more than a grid's y or z dimension holds.  The trio
    pass walks the words inside the kernel; the image kernel takes one workgroup a word in gridDim.x."""
    from eagleeverything_amd import r_api, rcpp_api
    L = 64 * R.GRID_Y + 65
    nwords = (L + 63) // 64
    assert nwords == 65537 > R.GRID_Y and L - 1 == 64 * 65536
    rng = np.random.default_rng(13)
    g = rng.integers(-1, 2, size=(L, 2)).astype(np.int8)
    g = np.concatenate((g, R.children(g, [(0, 1)], seed=3)), axis=1)
    planted = np.unique([64 * 65534 + 3, 64 * 65535 - 1, 64 * 65535, 64 * 65535 + 63, 64 * 65536, L - 1])     # the last word holds one marker
    g[planted] = (0, -1, 0)                              # a het father passes A2 to the het child of a hom A1 mother
    Mf = write_M(tmp_path, g)
    rcpp_api.drop_cache()
    trios = np.array([(2, 0, 1)], dtype=np.int32)
    want = r_api.tdt_host(g, None, trios, seed=1, R=2)
    got = rcpp_api.tdt(Mf, (3, L), trios, seed=1, R=2)
    T.same(got, want, "65,537 words")
    assert (got["marker"][planted] == (1, 0, 0, 0, 0)).all() and (got["key_obs"][planted] == 1.0).all() and got["trio"][0, 0] == L
    # one family: every flip is +-d_obs
    assert (got["count1"] == 2).all() and (got["maxkey"] == got["key_obs"].max()).all() and (got["argmax"] == got["key_obs"].argmax()).all()
    rcpp_api.drop_cache()
