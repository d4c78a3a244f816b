"""W = S (V S) on the int8 engine against an exact integer truth with a NON-diagonal S (tests/exact_w8.py, pinned on the CPU by
tests/test_w8_exact_host.py).

The operands are symmetric integer matrices whose digit planes the engine holds exactly and whose non-empty plane pairs lie inside the
configuration that ran -- read back and asserted, never assumed -- so the digit slicing, the per-row exponents, the work lists over tile
pairs and level groups, the k_w8_gemm* kernels, the level combine and the element-wise terms of k_w8_combine1 / 2 have nothing to lose:
the WHOLE folded image, X = S V^T and v = S a_hat are compared with array equality, on both tile engines, with the products cut into row
panels, on the fp64 products (exact on the same operands: k_gemm_f64_dma at a non-diagonal S), after the overflow fallback
(eagle_w8_redo_f64), and m^T S (V (S m)) of the re-evaluation path (eagle_w8_true_vara / k_w8_mgemv_part) for marker rows in {-1, 0, 1}^n:
exact_w8.check_exact proves 1^T |S| |V| |S| 1 < 2^53, so EVERY such row is exact, whatever the order -- the all +1, all -1, unit and
last-individual rows and the random ones alike.  A decline fails the test; nothing is skipped.

Not here: the row-sum vector r = S (V (S 1)) stays in the engine's workspace (the shard does not expose it; exact_w8 returns its truth
for the day it does), and the pipelined upload through the C ABI is pinned bit for bit to the non-pipelined call by
tests/test_gpu_w8.py::test_reference_shaped_call_on_the_int8_w -- not repeated."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from eagleeverything_amd._lib import TUNE

import exact_w8 as ex

pytestmark = pytest.mark.gpu
L_MARKERS = 129
# n: degenerate (no / one off-diagonal entry), around the 256- and 384-row tiles, several tiles, the last row of a 1,024 pad, and 1,537:
# n_pad = 1,792 = seven row tiles, five column tiles of 384 the last of which is short
CASES = [(1, "s1"), (2, "s1"), (255, "s1"), (256, "s1"), (257, "s1"), (257, "s2"), (383, "s1"), (385, "s1"), (385, "s2"), (640, "s1"),
         (1003, "s1"), (1003, "s2"), (1537, "s1"), (1537, "s2")]
PANELS = (1003, 1537)


@pytest.fixture(scope="module")
def api():
    from eagleeverything_amd import rcpp_api
    assert rcpp_api.device_info()["arch"].startswith("gfx950")
    yield rcpp_api
    rcpp_api.close_all()


@functools.lru_cache(maxsize=None)
def _case(n, kind):
    """(operands, truth): built and bounded once per module in integers, read-only from then on."""
    case = ex.build_case(n, kind)
    truth = ex.check_exact(case)
    for d in (case, truth):
        for x in d.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return case, truth


def _shard(case, L=L_MARKERS):
    import torch
    from eagleeverything_amd.sharded import DeviceShard
    sh = DeviceShard(case["n"], L)
    n = case["n"]
    sh.set_operands(case["S"][:n, :n].copy(), case["V"][:n, :n].copy(), case["ahat"][:n].copy())
    sh.mode = 1
    sh.L.eagle_dev_set_spectral(sh.ctx, 0)
    return torch, sh


def _rows_of(case, i):
    """e_i and the non-empty planes of row i of S, V and X, for the failure message."""
    out = []
    for name, M in (("S", case[0]["Si"]), ("V", case[0]["Vi"]), ("X", case[1]["X"])):
        e, d = ex.planes(M)
        out.append("%s: e=%d planes=%s" % (name, e[i], [p + 1 for p in range(ex.KMAX) if d[p][i].any()]))
    return "; ".join(out)


def _assert_image(dev, want, both, what):
    """array equality over all n_pad x n_pad; the first wrong element names itself: its tile pair, the planes of its two rows."""
    got = dev.cpu().numpy()
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    j, k = (int(x) for x in bad[0])
    n = both[0]["n"]
    rows = " | ".join("row %d: %s" % (i, _rows_of(both, i)) for i in (j, k) if i < n)
    raise AssertionError("%s: %d wrong elements, first [%d][%d] = %r, truth %r; 256-tile pair (%d, %d), 384-column tile %d; %s"
                         % (what, len(bad), j, k, got[j, k], want[j, k], j // 256, k // 256, k // 384, rows))


def _int8_products(torch, sh, both, what):
    case, truth = both
    sh.w_mode = 2
    sh.scan_operands()
    torch.cuda.synchronize()
    info = sh.w_info()
    assert info["int8"] == 1 and info["declined"] == 0, (what, info)         # a decline is a failure, never a skip
    assert ex.covered(truth["pairs1"], info["k1"], info["T1"]), (what, sorted(truth["pairs1"]), info)
    assert ex.covered(truth["pairs2"], info["k2"], info["T2"]), (what, sorted(truth["pairs2"]), info)
    assert info["asym_term"] == 0.0, (what, info)
    _assert_image(sh.tmp, truth["tmp"], both, what + ": X = S V^T")
    _assert_image(sh.Wu, truth["Wu"], both, what + ": folded W")               # nothing below the diagonal, zeros in the padding
    assert np.array_equal(sh.v.cpu().numpy(), truth["vv"]), what + ": v = S a_hat"
    return info


def _level_groups(k, T, np_):
    """Accumulation groups of configuration (k, T) (w8_groups): the pairs of one level, at most min(8, 131071 / n_pad) per group."""
    maxp = min(8, 131071 // np_)
    return sum(-(-sum(1 for p in range(1, k + 1) if 1 <= t - p <= k) // maxp) for t in range(2, T + 1))


def _row_panels(k, T, np_, mb):
    """Row panels of one product when the level images get `mb` MB (the rule of w8_product): whole row tiles per panel, whole
    super-tile rows of 8 (4) above that."""
    nt = np_ // 256
    level_bytes = min(12 * np_ * np_ * 4, mb << 20)
    per = level_bytes // (_level_groups(k, T, np_) * 256 * np_ * 4)
    assert per >= 1
    if per >= nt:
        per = nt
    elif per > 8:
        per = per // 8 * 8
    elif per > 4:
        per = 4
    return -(-nt // per)


@pytest.mark.parametrize("n,kind", CASES)
def test_int8_w_is_the_integer_truth_on_both_engines_and_in_row_panels(n, kind, api):
    both = _case(n, kind)
    torch, sh = _shard(both[0])
    what = "n=%d %s" % (n, kind)
    try:
        info = _int8_products(torch, sh, both, what + " 384 x 256 engine")
        sh.L.eagle_dev_set_tune(sh.ctx, TUNE["W8_UNPIPED"])
        _int8_products(torch, sh, both, what + " 256 x 256 engine")
        if n in PANELS:   # room for the level images of two row tiles: at least two row panels in both products, on either engine
            groups = max(_level_groups(info["k1"], info["T1"], sh.np_), _level_groups(info["k2"], info["T2"], sh.np_))
            mb = max(1, (groups * 256 * sh.np_ * 4 * 2) >> 20)
            os.environ["EAGLE_HIP_W8_LEVEL_MB"] = str(mb)
            for k, T in ((info["k1"], info["T1"]), (info["k2"], info["T2"])):
                assert _row_panels(k, T, sh.np_, mb) >= 2, (k, T, mb)
            _int8_products(torch, sh, both, what + " 256 x 256 engine, row panels")
            sh.L.eagle_dev_set_tune(sh.ctx, TUNE["SHIPPED"])
            _int8_products(torch, sh, both, what + " 384 x 256 engine, row panels")
    finally:
        os.environ.pop("EAGLE_HIP_W8_LEVEL_MB", None)
        sh.L.eagle_dev_set_tune(sh.ctx, TUNE["SHIPPED"])
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)


@pytest.mark.parametrize("n,kind", CASES)
def test_fp64_products_are_the_integer_truth(n, kind, api):
    both = _case(n, kind)
    case, truth = both
    torch, sh = _shard(case)
    try:
        sh.w_mode = 0
        sh.scan_operands()
        torch.cuda.synchronize()
        info = sh.w_info()
        assert info["int8"] == 0 and info["declined"] == 7, info
        what = "fp64 n=%d %s" % (n, kind)
        # (the fp64 products leave the other factor order in tmp: V S, the transpose of the int8 path's X = S V^T -- the same integers)
        _assert_image(sh.tmp, np.ascontiguousarray(truth["tmp"].T), both, what + ": V S")
        _assert_image(sh.Wu, truth["Wu"], both, what + ": folded W")
        assert np.array_equal(sh.v.cpu().numpy(), truth["vv"])
    finally:
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)


def _marker_rows(n, np_, count, seed):
    """All +1, all -1, the unit row e_0, a row that is non-zero only in the last individual, then random genotypes."""
    rng = np.random.default_rng(seed)
    M = np.zeros((count, np_), dtype=np.int8)
    M[:, :n] = rng.integers(-1, 2, size=(count, n))
    M[0, :n] = 1
    M[1, :n] = -1
    M[2, :n] = 0
    M[2, 0] = 1
    M[3, :n] = 0
    M[3, n - 1] = -1
    return M


@pytest.mark.parametrize("n,kind", [(2, "s1"), (257, "s2"), (385, "s1"), (1003, "s2"), (1537, "s1")])
def test_re_evaluation_is_the_integer_truth(n, kind, api):
    """eagle_w8_true_vara on the operands the int8 call left on record, for rows of the shard's genotype image: 16 in order (one MFMA row
    tile per pass) and 40 scattered through a destination index as the certificate does (four row tiles), equal to m^T S (V (S m)) in
    integers for every row (see the module docstring for why every row is exact)."""
    both = _case(n, kind)
    case, truth = both
    torch, sh = _shard(case)
    fn = sh.L.eagle_w8_true_vara
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]
    try:
        _int8_products(torch, sh, both, "n=%d %s" % (n, kind))
        for count in (16, 40):
            M = _marker_rows(n, sh.np_, count, seed=n + count)
            want = ex.vara_truth(case, M[:, :n]).astype(np.float64)
            sh.Mt8[:count] = torch.from_numpy(M).to(sh.dev)                # the rows of the shard's own genotype image
            sh.vara.fill_(-1.0)
            if count == 16:   # in order, no index
                sh._check(fn(sh.ctx, sh.Mt8.data_ptr(), count, sh.np_, sh.np_, None, sh.vara.data_ptr(), sh._stream()))
                where = np.arange(count)
            else:             # scattered through the index the certificate hands over
                where = (7 * np.arange(count) + 3) % L_MARKERS
                dst = torch.from_numpy(where.astype(np.int64)).to(sh.dev)
                sh._check(fn(sh.ctx, sh.Mt8.data_ptr(), count, sh.np_, sh.np_, dst.data_ptr(), sh.vara.data_ptr(), sh._stream()))
            torch.cuda.synchronize()
            allv = sh.vara.cpu().numpy()
            got = allv[where]
            assert np.array_equal(got, want), (count, np.flatnonzero(got != want)[:8], got[:4], want[:4])
            assert np.count_nonzero(allv != -1.0) <= count                   # nothing written elsewhere
            assert want[0] == want[1] == float(truth["W"].sum()) and want[2] == float(truth["W"][0, 0]) and want[3] == float(truth["W"][n - 1, n - 1])
    finally:
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)


def test_overflow_fallback_leaves_the_integer_truth(api):
    """eagle_w8_redo_f64: three forced slices cannot certify a W whose diagonal spans 2^50 -- more than 2,048 markers are flagged, the
    certificate overflows (as in test_gpu_w8.py::test_an_overflowing_certificate_replaces_the_int8_w_by_the_fp64_products) and the fp64
    products replace the image in place: the same truth."""
    both = _case(385, "s1")
    case, truth = both
    L = 2304
    torch, sh = _shard(case, L)
    rng = np.random.default_rng(5)
    sh.Mt8[:L, :case["n"]] = torch.from_numpy(rng.integers(-1, 2, size=(L, case["n"])).astype(np.int8)).to(sh.dev)
    try:
        sh.w_mode, sh.nslices = 2, 3
        sh.scan()
        torch.cuda.synchronize()
        assert sh.certificate()["overflow"] == 1, sh.certificate()
        info = sh.w_info()
        assert info["int8"] == 0 and info["declined"] == 8, info
        _assert_image(sh.Wu, truth["Wu"], both, "after eagle_w8_redo_f64")
        assert np.array_equal(sh.v.cpu().numpy(), truth["vv"])
    finally:
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)
