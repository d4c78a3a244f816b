"""CPU: linkage disequilibrium without a device -- the two entry points are declared, exported and bound; the greedy pruning rule
(r_api.ld_prune_keep) on hand-made masks; r^2 from integer dot products (r_api.ld_r2_from_dots) against np.corrcoef; argument errors
that are decided before a device is needed.  Expected values are written here by hand or restated in numpy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3


def make_mask(L, window, pairs):
    """The (L, ceil(window / 64)) uint64 mask eagle_ld_window would return for the pairs (i, j), 0 < j - i <= window."""
    m = np.zeros((L, (window + 63) // 64), dtype=np.uint64)
    for i, j in pairs:
        o = j - i
        assert 1 <= o <= window and j < L
        m[i, (o - 1) // 64] |= np.uint64(1) << np.uint64((o - 1) % 64)
    return m


def greedy(L, pairs, order):
    """Plain-loop restatement: visit in `order`, keep a marker unless a kept marker is paired with it."""
    adj = [set() for _ in range(L)]
    for i, j in pairs:
        adj[i].add(j)
        adj[j].add(i)
    keep = np.zeros(L, dtype=bool)
    for i in order:
        keep[i] = not any(keep[j] for j in adj[i])
    return keep


# ------------------------------------------------------------------------------------------------ 1. the ABI
def test_ld_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, am, r_api, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eagle_hip.h")).read(), flags=re.S)
    L = _lib.load()
    for name, nargs in (("eagle_ld_window", 8), ("eagle_ld_dots", 7)):
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert _lib.SIGNATURES[name][0] is C.c_int and len(_lib.SIGNATURES[name][1]) == nargs
    for mod, names in ((rcpp_api, ("ld_window", "ld_dots")), (r_api, ("ld_r2_from_dots", "ld_prune_keep", "LDPrune", "LDofLoci")),
                       (am, ("tag_markers",))):
        for name in names:
            assert callable(getattr(mod, name))


# ------------------------------------------------------------------------------------------------ 2. the greedy rule
def test_prune_chain_position_and_priority():
    from eagleeverything_amd import r_api
    m = make_mask(3, 2, [(0, 1), (1, 2)])                                   # A-B, B-C, not A-C
    assert r_api.ld_prune_keep(m, 2).tolist() == [True, False, True]       # index order: A stays, B goes, C has no kept partner
    assert r_api.ld_prune_keep(m, 2, priority=[0.1, 0.4, 0.2]).tolist() == [False, True, False]   # B first: it removes both
    assert r_api.ld_prune_keep(m, 2, priority=[0.3, 0.1, 0.2]).tolist() == [True, False, True]


def test_prune_chromosome_and_kb_cuts():
    from eagleeverything_amd import r_api
    m = make_mask(4, 3, [(0, 1), (1, 2), (2, 3)])
    assert r_api.ld_prune_keep(m, 3).tolist() == [True, False, True, False]
    assert r_api.ld_prune_keep(m, 3, chrom=["1", "1", "2", "2"]).tolist() == [True, False, True, False]   # 1-2 is cut: 2 starts anew
    assert r_api.ld_prune_keep(m, 3, chrom=["1", "2", "2", "3"]).tolist() == [True, True, False, True]
    pos = [1000, 2000, 52000, 52001]
    assert r_api.ld_prune_keep(m, 3, pos=pos, kb=50).tolist() == [True, False, True, False]                 # exactly 50 kb counts
    assert r_api.ld_prune_keep(m, 3, pos=[0, 1000, 51000, 200000], kb=50).tolist() == [True, False, True, True]   # 2-3 is cut
    two = make_mask(3, 1, [(0, 1)])
    assert r_api.ld_prune_keep(two, 1, pos=[0, 50000, 50001], kb=50).tolist() == [True, False, True]
    assert r_api.ld_prune_keep(two, 1, pos=[0, 50001, 50002], kb=50).all()                                  # one base pair too far
    assert r_api.ld_prune_keep(two, 1, pos=[50001, 0, 7], kb=50).all()                                      # the distance is absolute
    assert r_api.ld_prune_keep(m, 3, chrom=[1, 1, 1, 1], pos=[0, 60000, 120000, 180000], kb=50).all()
    with pytest.raises(ValueError):
        r_api.ld_prune_keep(m, 3, kb=50)


def test_prune_pair_at_distance_exactly_window():
    from eagleeverything_amd import r_api
    for window in (1, 64, 65, 256):
        L = window + 3
        keep = r_api.ld_prune_keep(make_mask(L, window, [(1, 1 + window)]), window)
        assert np.flatnonzero(~keep).tolist() == [1 + window]
        keep = r_api.ld_prune_keep(make_mask(L, window, [(1, 1 + window)]), window, priority=np.arange(L))
        assert np.flatnonzero(~keep).tolist() == [1]
    with pytest.raises(ValueError):                                         # a mask of the wrong width is refused, not misread
        r_api.ld_prune_keep(make_mask(70, 65, []), 64)


def test_prune_tie_break_and_empty_mask():
    from eagleeverything_amd import r_api
    m = make_mask(4, 1, [(0, 1), (2, 3)])
    assert r_api.ld_prune_keep(m, 1, priority=[0.5, 0.5, 0.2, 0.7]).tolist() == [True, False, False, True]   # tie 0 / 1: the index
    assert r_api.ld_prune_keep(m, 1, priority=[np.nan, 0.0, 0.2, 0.2]).tolist() == [False, True, True, False]  # NaN is visited last
    assert r_api.ld_prune_keep(make_mask(7, 50, []), 50).all()
    assert r_api.ld_prune_keep(make_mask(7, 50, []), 50, priority=np.arange(7)).all()
    assert r_api.ld_prune_keep(np.zeros((0, 1), dtype=np.uint64), 50).shape == (0,)


def test_prune_equals_the_plain_loop_on_random_masks():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(7)
    for window in (3, 70):
        L = 300
        pairs = sorted({(int(i), int(i + o)) for i, o in zip(rng.integers(0, L, 400), rng.integers(1, window + 1, 400)) if i + o < L})
        m = make_mask(L, window, pairs)
        assert np.array_equal(r_api.ld_prune_keep(m, window), greedy(L, pairs, range(L)))
        pr = rng.integers(0, 20, L) / 40.0                                  # many ties
        order = sorted(range(L), key=lambda i: (-pr[i], i))
        assert np.array_equal(r_api.ld_prune_keep(m, window, priority=pr), greedy(L, pairs, order))


# ------------------------------------------------------------------------------------------------ 3. r^2 from dot products
def test_r2_from_dots_against_corrcoef():
    from eagleeverything_amd import r_api
    rng = np.random.default_rng(3)
    G = rng.integers(-1, 2, (40, 30)).astype(np.int64)                      # 40 individuals x 30 markers
    G[:, 4] = 1
    G[:, 17] = 0                                                            # two monomorphic markers, one of them among the loci
    G[:, 9] = G[:, 2]
    G[:, 11] = -G[:, 2]
    loci = [2, 17, 29, 2]
    dots = (G.T @ G)[:, loci]
    st = r_api.marker_stats_from_counts((G == -1).sum(0), (G == 0).sum(0), (G == 1).sum(0))
    r2 = r_api.ld_r2_from_dots(dots, st, loci, 40)
    assert r2.shape == (30, 4) and r2.dtype == np.float64
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = np.corrcoef(G.T.astype(np.float64)) ** 2
    mono = np.zeros(30, dtype=bool)
    mono[[4, 17]] = True
    assert np.isnan(r2[mono]).all() and np.isnan(r2[:, 1]).all()
    ok = ~mono[:, None] & ~mono[loci][None, :]
    assert not np.isnan(r2[ok]).any() and np.max(np.abs(r2[ok] - ref[:, loci][ok])) < 1e-12
    assert r2[2, 0] == 1.0 and r2[9, 0] == 1.0 and r2[11, 3] == 1.0 and r2[29, 2] == 1.0


# ------------------------------------------------------------------------------------------------ 4. errors that need no device
def test_ld_argument_errors_without_a_device(tmp_path):
    from eagleeverything_amd import _lib, rcpp_api
    from eagleeverything_amd._lib import c_lp
    L = _lib.load()
    f = os.fsencode(str(tmp_path / "Mt.ascii"))
    dims = (C.c_long * 2)(150, 100)
    mask = (C.c_uint64 * 400)()
    pairs = C.c_long(0)
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)

    def win(window, r2, f=f, dims=dims, mask=mask, pairs=C.byref(pairs)):
        rc = L.eagle_ld_window(None, f, dims, window, r2, 8.0, C.cast(mask, u64p) if mask is not None else None, pairs)
        return rc, L.eagle_open_error().decode()
    for window in (0, -1, 257):
        rc, text = win(window, 0.2)
        assert rc == ERR_ARG and "window" in text, (window, text)
    for r2 in (-0.001, 1.0001, float("nan"), float("inf")):
        rc, text = win(50, r2)
        assert rc == ERR_ARG and "r2" in text, (r2, text)
    for kw in ({"f": None}, {"dims": None}, {"mask": None}, {"pairs": None}):
        rc, text = win(50, 0.2, **kw)
        assert rc == ERR_ARG and "NULL" in text, (kw, text)
    rc, text = win(50, 0.2, dims=(C.c_long * 2)(0, 100))
    assert rc == ERR_ARG and "positive" in text
    for window, r2 in ((1, 0.0), (256, 1.0), (50, 0.2)):                   # good arguments get as far as asking for the context
        rc, text = win(window, r2)
        assert rc == ERR_ARG and "no context" in text

    dots = (C.c_int32 * (100 * 64))()

    def dot(loci, nloci=None, f=f, dims=dims, out=dots, null_loci=False):
        lv = np.zeros(max(len(loci), 1), dtype=np.int64)
        lv[:len(loci)] = loci
        rc = L.eagle_ld_dots(None, f, dims, None if null_loci else lv.ctypes.data_as(c_lp), len(loci) if nloci is None else nloci, 8.0,
                             C.cast(out, i32p) if out is not None else None)
        return rc, L.eagle_open_error().decode()
    for loci, nloci in (([], None), ([1], 0), ([1], -2), (list(range(65)), None)):
        rc, text = dot(loci, nloci)
        assert rc == ERR_ARG and "number of loci" in text, (loci, text)
    for loci in ([100], [-1], [3, 99, 100]):
        rc, text = dot(loci)
        assert rc == ERR_ARG and "outside" in text, (loci, text)
    for kw in ({"f": None}, {"dims": None}, {"out": None}, {"null_loci": True}):
        rc, text = dot([1, 2], **kw)
        assert rc == ERR_ARG and "NULL" in text, (kw, text)
    for loci in ([0], [99, 99, 0], list(range(64))):
        rc, text = dot(loci)
        assert rc == ERR_ARG and "no context" in text
    if 0 not in rcpp_api._ctx:   # the Python bindings report the same errors without opening a device
        for call in (lambda: rcpp_api.ld_window(str(tmp_path / "Mt.ascii"), (150, 100), 300, 0.2),
                     lambda: rcpp_api.ld_window(str(tmp_path / "Mt.ascii"), (150, 100), 50, 1.5),
                     lambda: rcpp_api.ld_dots(str(tmp_path / "Mt.ascii"), (150, 100), [100]),
                     lambda: rcpp_api.ld_dots(str(tmp_path / "Mt.ascii"), (150, 100), [])):
            with pytest.raises(rcpp_api.EagleError) as e:
                call()
            assert e.value.code == ERR_ARG and "no context" not in e.value.text
        assert 0 not in rcpp_api._ctx
    assert sorted(os.listdir(tmp_path)) == []


def test_ldprune_host_exits(tmp_path):
    """LDPrune decides these on the host, before any device call: a bad prefer, kb without a map, a map of the wrong length, an
    outdir that holds the source."""
    from eagleeverything_amd import r_api
    src = tmp_path / "src"
    src.mkdir()
    geno = {"asciifileM": str(src / "M.ascii"), "asciifileMt": str(src / "Mt.ascii"), "dim_of_ascii_M": [150, 100]}
    for kw, word in (({"prefer": "best"}, "prefer"), ({"kb": 10}, "kb= needs a map"),
                     ({"map": {"SNP": ["a"], "Chr": ["1"], "Pos": [1]}}, "names 1 markers"), ({"map": ["a"] * 100}, "Chr and Pos"),
                     ({"outdir": str(src)}, "directory of their own")):
        msgs = []
        assert r_api.LDPrune(geno, message=msgs.append, **kw) is None
        assert any(word in m for m in msgs) and "LDPrune has terminated with errors" in msgs[-1], (kw, msgs)
    assert os.listdir(src) == []
