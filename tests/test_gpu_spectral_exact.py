"""The eigenbasis scan against an exact dyadic truth (tests/exact_spectral.py, pinned on the CPU by tests/test_spectral_exact_host.py).

With a block-Hadamard U, power-of-two d_k, integer U^T y and U^T X columns of disjoint support, Z = Mt U, lin, quad, a, vara and every
partial sum a kernel can form are dyadic rationals that fp64 holds, so k_zbuild, the int8 digit-slice Z build, k_spectral_scan<1|2>,
k_spectral_finish, k_spectral_scan_traits<2..8> and k_spectral_finish_traits must return the truth's bits in whatever order they sum:
every comparison below is an equality (the arg-max VALUE alone is held to 2 ulp, the margin of tests/test_gpu_scan_exact.py).  A k
dropped at a chunk edge, a pad column read as data, a quad column taken from the neighbouring trait or a row tile written to the wrong 16
markers passes the tolerance tests of this suite and a comparison of two paths that share it; here it fails with a marker index.

eagle_last_scan_argmax is defined on the last eagle_calculate_a_and_vara call and does not see a spectral scan; the single scan's arg-max is
taken as am.SpectralBackend.find_qtl takes it (on the returned arrays) and on the device through a one-trait eagle_spectral_scan_traits."""
import functools

import numpy as np
import pytest

import exact_spectral as xs
from eagleeverything_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from eagleeverything_amd import rcpp_api
    assert rcpp_api.device_info()["arch"].startswith("gfx950")
    yield rcpp_api
    rcpp_api.close_all()


@functools.lru_cache(maxsize=None)
def _case(n, L):
    """Built once, never written to."""
    case = xs.build_case(n, L)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _single(n, L, p, sel=()):
    case = _case(n, L)
    op = xs.single_op(case, p)
    xs.check_exact(case, op)                                             # Python ints: every partial sum is a double, before the device is asked
    return op, xs.truth(case, op, sel=sel)


def _prepare(api, case, tmp_path, device=0):
    geno = synth.write_geno_pair(str(tmp_path), case["Mt8"], stem="d%s" % (device != 0))
    api.spectral_prepare(geno["asciifileMt"], (case["L"], case["n"]), case["U"], 8.0, device=device)


def _single_scans(api, case, device=0):
    """(b): both entry points at every p the case has room for; -> {p: (a, vara)}."""
    n, L = case["n"], case["L"]
    out = {}
    for p in xs.single_ps(case):
        op, tr = _single(n, L, p)
        what = "n=%d L=%d p=%d" % (n, L, p)
        UtX, Uty = op["X"].astype(np.float64), op["y"].astype(np.float64)
        r1 = api.spectral_scan(case["lam"], UtX, Uty, op["varE"], op["varG"], L, device=device)
        xs.assert_scan(r1["a"], r1["vara"], tr, what + " spectral_scan")
        xs.assert_planted(r1["a"], r1["vara"], case, op, tr, what)
        r2 = api.spectral_scan_weights(op["d"], op["d"] * Uty, op["d"][:, None] * UtX, op["C"], op["c1"], op["varG"], L, device=device)
        xs.assert_scan(r2["a"], r2["vara"], tr, what + " spectral_scan_weights")
        np.testing.assert_array_equal(r1["a"], r2["a"])
        np.testing.assert_array_equal(r1["vara"], r2["vara"])
        xs.assert_argmax(*xs.host_argmax(r1["a"], r1["vara"]), tr, what + " arg-max of the returned arrays")
        one = api.spectral_scan_traits(case["lam"], [UtX], Uty, [op["varE"]], [op["varG"]], L, device=device)
        xs.assert_argmax(one["index"][0], one["tsqmax"][0], tr, what + " arg-max on the device")
        # selected_loci: exact zeros at exactly those rows, everything else untouched, the arg-max moves off the masked first of the pair
        sel = tuple(sorted({0, L // 2, L - 1}))
        _, trm = _single(n, L, p, sel)
        rm = api.spectral_scan(case["lam"], UtX, Uty, op["varE"], op["varG"], L, selected_loci=np.array(sel, dtype=np.float64), device=device)
        xs.assert_scan(rm["a"], rm["vara"], trm, what + " masked")
        xs.assert_planted(rm["a"], rm["vara"], case, op, trm, what + " masked", sel=sel)
        xs.assert_argmax(*xs.host_argmax(rm["a"], rm["vara"]), trm, what + " masked arg-max")
        out[p] = (r1["a"].copy(), r1["vara"].copy())
    return out


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("n,L", xs.SHAPES)
def test_z_and_single_scan_are_the_dyadic_truth(n, L, mode, api, tmp_path):
    """(a), (b): Z from the digit-slice build (mode 1, the default) and from k_zbuild (mode 0), every element; then k_spectral_scan<1> (p = 1,
    15), k_spectral_scan<2> (p = 16, 31) and k_spectral_finish through both entry points on that Z."""
    case = _case(n, L)
    try:
        api.set_scan_mode(mode)
        _prepare(api, case, tmp_path)
        Z = api.spectral_rows(np.arange(L))
        assert Z.shape == (n, L)
        xs.assert_z(Z.T, case, "n=%d L=%d scan mode %d" % (n, L, mode))
        _single_scans(api, case)
    finally:
        api.set_scan_mode(1)
        api.drop_cache()


def _batched(api, case, device=0, lists=xs.TRAIT_LISTS):
    """(c): every trait list; -> [result of full=True]."""
    n, L = case["n"], case["L"]
    outs = []
    for k, (plist, widths) in enumerate(lists):
        assert [g[3] for g in xs.trait_groups(plist)] == widths
        assert api.spectral_traits_passes(plist) == len(widths)
        ops = [xs.trait_op(case, t, p) for t, p in enumerate(plist)]
        UtX = [op["X"].astype(np.float64) for op in ops]
        UtY = np.column_stack([op["y"] for op in ops]).astype(np.float64)
        vE, vG = [op["varE"] for op in ops], [op["varG"] for op in ops]
        res = api.spectral_scan_traits(case["lam"], UtX, UtY, vE, vG, L, full=True, device=device)
        assert res["a"].shape == res["vara"].shape == (L, len(plist))
        for t, op in enumerate(ops):
            what = "n=%d L=%d list %d trait %d (p=%d)" % (n, L, k, t, plist[t])
            xs.check_exact(case, op)
            tr = xs.truth(case, op)
            xs.assert_scan(res["a"][:, t], res["vara"][:, t], tr, what)
            xs.assert_planted(res["a"][:, t], res["vara"][:, t], case, op, tr, what)
            xs.assert_argmax(res["index"][t], res["tsqmax"][t], tr, what)
        lean = api.spectral_scan_traits(case["lam"], UtX, UtY, vE, vG, L, device=device)
        np.testing.assert_array_equal(lean["index"], res["index"])
        np.testing.assert_array_equal(lean["tsqmax"], res["tsqmax"])
        outs.append(res)
    return outs


@pytest.mark.parametrize("n,L", xs.TRAIT_SHAPES)
def test_batched_scan_every_group_width_is_the_dyadic_truth(n, L, api, tmp_path):
    """(c): k_spectral_scan_traits<NT> for NT = 2..8 (KC = 256, 128, 64: 1 to 16 chunks) and k_spectral_finish_traits; the traits of a group
    differ in d, p, Uty and their columns of U^T X."""
    case = _case(n, L)
    try:
        _prepare(api, case, tmp_path)
        _batched(api, case)
    finally:
        api.drop_cache()


def test_two_contexts_on_one_card_are_the_dyadic_truth(api, tmp_path):
    """(d): the markers split over two contexts of the card at 512 of 1,000: the truth again, bit for bit the one-context run, and the
    duplicated pair (markers 1 and 1,000, one per shard) resolves to the smaller global index."""
    n, L = 1003, 1000
    case = _case(n, L)
    lists = xs.TRAIT_LISTS[:1]
    res = {}
    try:
        for dev in (0, (0, 0)):
            _prepare(api, case, tmp_path, device=dev)
            Z = api.spectral_rows(np.array([0, 511, 512, L - 1]), device=dev)
            np.testing.assert_array_equal(Z.T, case["Z"][[0, 511, 512, L - 1]])
            res[dev] = (_single_scans(api, case, device=dev), _batched(api, case, device=dev, lists=lists))
    finally:
        for dev in (0, (0, 0)):
            if dev in api._ctx:
                api.drop_cache(device=dev)
    for p, (a, v) in res[0][0].items():
        np.testing.assert_array_equal(a, res[(0, 0)][0][p][0])
        np.testing.assert_array_equal(v, res[(0, 0)][0][p][1])
    for r0, r1 in zip(res[0][1], res[(0, 0)][1]):
        for key in ("a", "vara", "index", "tsqmax"):
            np.testing.assert_array_equal(r0[key], r1[key], err_msg=key)
    _, tr = _single(n, L, 31)
    assert case["dup"] == (0, L - 1) and tr["argmax"][0] == 1             # what _single_scans held the device arg-max of both runs to
