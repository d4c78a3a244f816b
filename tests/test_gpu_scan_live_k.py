"""k_vara_i8p on the LOWER image of the digit slices: every K loop ends at the last live stage of W (csrc/eagle_i8mfma.hip: k_slice_w's
klive and lower layout, VaraIt; the walk itself is restated on the host by tests/test_scan_live_k_host.py).

The kernel sums the same integer products in another order and leaves out stages that hold only zeros, so the int64 q block, vara and
the live-stage count are compared by equality and nothing else: against the same build in the parent's order (VARA_UPPER), against the
compiler-scheduled kernel on the untransposed-row layout (COMPILER_SCHEDULED), under the paced form (VARA_PACED), and against the integer truth of
tests/exact_scan.py.  W is handed over ready-made (DeviceShard.set_W): the dense W of an exact_scan case; the same with the off-diagonals
of the last live individuals zeroed (klive below ceil(n / 128)); its diagonal alone (klive = 0: every tile on the two-stage floor); and a
single off-diagonal entry at (0, n-1).  n -> n_pad: 120 -> 256 (one tile, pad >= 128: the floor binds), 130 -> 256 (pad < 128), 300 -> 512
(zeroed tail: the last tile wholly above klive), 600 -> 768 (one stage dropped from tiles 0 and 1, the floor on tile 2), 700 -> 768 and
1,003 -> 1,024 (nothing dropped).  L = 1,003: two marker tiles of 384 and a ragged one.  Then the extension's launch on the compact image
(its second header holds no count) and a streamed scan whose second marker block must still see the count of the W-dependent part."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import exact_lastdigit as xl
import exact_scan as ex
from eagleeverything_amd._lib import TUNE

pytestmark = pytest.mark.gpu
L = 1003
SHAPES = [120, 130, 300, 600, 700, 1003]
DESIGNS = ("dense", "tail0", "diag", "corner")
POISON = 0xA5
SHIPPED, UPPER, COMPILER, PACED = TUNE["SHIPPED"], TUNE["VARA_UPPER"], TUNE["COMPILER_SCHEDULED"], TUNE["VARA_PACED"]


@functools.lru_cache(maxsize=None)
def _base(n, S):
    case = ex.build_case(n, L, log2u=ex.LOG2U_OF_SLICES[S])
    ex.check_exact(case)
    case["X"].setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _designed(n, S, design):
    """(case with the designed X, a, vara, klive): off-diagonals only ever removed or replaced by the case's own largest entry, the
    dominant diagonal kept -- the exactness bound of the base case (check_exact) covers every design."""
    base = _base(n, S)
    X = base["X"].copy()
    d = np.diag(np.diag(X))
    if design == "tail0":
        t = min(200, n // 2)
        X[n - t:, :] = 0
        X[:, n - t:] = 0
        X += d - np.diag(np.diag(X))
    elif design == "diag":
        X = d
    elif design == "corner":
        X = d.copy()
        X[0, n - 1] = X[n - 1, 0] = ex.MAXOFF << -base["log2u"]
    case = dict(base, X=X, max_pair=None)
    a, vara, _ = ex.scan_truth(case)
    return case, a, vara, _klive(np.triu(X, 1))


def _klive(upper):
    """k_slice_w: (largest column j holding a non-zero entry above the diagonal) / 128 + 1; 0 without one."""
    cols = np.flatnonzero(np.asarray(upper != 0).any(axis=0))
    return int(cols[-1]) // 128 + 1 if cols.size else 0


def _tune(sh, v):
    sh.L.eagle_dev_set_tune(sh.ctx, int(v))


def _kernel(torch, sh, tune, smax):
    """prepare on a poisoned workspace + the vara kernel under `tune` -> (q block of all smax slots, vara, a, klive, S used, e)."""
    _tune(sh, tune)
    sh._ws().fill_(POISON)
    sh.vara_prepare()
    sh.vara_kernel()
    torch.cuda.synchronize()
    S_used = sh.vara_i8_info()[0]
    q = sh.ws[256:256 + 8 * smax * sh.Lp].view(torch.int64).clone()
    klive = int(sh.ws[128:132].view(torch.int32).item())
    return q, sh.vara[:sh.Lloc].clone(), sh.a[:sh.Lloc].clone(), klive, S_used, sh.last_e


def _assert_same(torch, got, ref, what):
    assert torch.equal(got[0], ref[0]), "q differs: " + what
    assert torch.equal(got[1], ref[1]), "vara differs: " + what
    assert got[3] == ref[3], ("klive", what, got[3], ref[3])


@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("n", SHAPES)
def test_lower_walk_is_the_upper_walk_and_the_integer_truth(n, S):
    import torch
    from eagleeverything_amd.sharded import DeviceShard
    sh = DeviceShard(n, L)
    sh.Mt8[:L, :n] = torch.from_numpy(_base(n, S)["Mt8"].copy()).to(sh.dev)
    sh.mode, sh.nslices = 1, S
    try:
        for design in DESIGNS:
            case, a, vara, klive = _designed(n, S, design)
            sh.set_W(np.ldexp(case["X"].astype(np.float64), case["log2u"]), case["ahat"])
            sh.scan_operands()
            out = {t: _kernel(torch, sh, t, S) for t in (SHIPPED, UPPER, COMPILER, PACED)}
            what = "n=%d S=%d %s" % (n, S, design)
            q0, v0, a0, kl, S_used, e = out[SHIPPED]
            print(what, "klive", kl, "of", sh.np_ // 128, "S used", S_used, "e", e)
            assert kl == klive, (what, kl, klive)
            assert S_used == (S if klive else 1)
            assert design == "diag" or int(q0.abs().max()) > 0
            for t in (UPPER, COMPILER, PACED):
                _assert_same(torch, out[t], out[SHIPPED], "%s, tune %d against the default" % (what, t))
            # the truth applies where the S digits hold W exactly: the unit of the last digit at or below the step 2 u of the folded entries
            assert klive == 0 or 2.0 ** (e + 2 - 8 * S_used) <= 2.0 * 2.0 ** case["log2u"], (what, e, S_used)
            np.testing.assert_array_equal(a0.cpu().numpy(), a, err_msg=what)
            bad = np.flatnonzero(v0.cpu().numpy() != vara)
            assert bad.size == 0, "%s: vara of %d markers, first %d: %r, truth %r" % (what, bad.size, bad[0], float(v0[bad[0]]), vara[bad[0]])
    finally:
        _tune(sh, SHIPPED)


def test_extension_launch_reads_the_workspace_count():
    """The spectral path at n = 300 -> 512 (klive = 3 of 4: tile 0 loses its last stage) with the compact image forced to 768 rows: the
    flagged markers get the dropped digit back and carry the truth, in both orders and on the old layout, bit for bit."""
    import torch
    from eagleeverything_amd.sharded import DeviceShard
    name = "S4-n300"
    n, Lc, S_wc, _, packed = xl.SCAN_CASES[name]
    case = xl.scan_case(name)
    _, vara, _ = ex.scan_truth(case)
    sh = DeviceShard(n, Lc)
    os.environ["EAGLE_HIP_EXT_CAP"] = "768"                                # (read when the workspace is sized and at every launch)
    try:
        sh.Mt8[:Lc, :n] = torch.from_numpy(case["Mt8"].copy()).to(sh.dev)
        sh.set_operands(case["S"], case["V"], case["ahat"])
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)
        sh._check(sh.L.eagle_set_scan_budget(sh.ctx, 0.0))
        sh.mode, sh.nslices, sh.packed, sh.certified = 1, 0, packed, False
        sh.scan_operands()
        torch.cuda.synchronize()
        klive = _klive(np.triu(sh.Wu.cpu().numpy(), 1))
        assert klive == 3 and sh.np_ == 512
        sh.extend = False
        raw = _kernel(torch, sh, SHIPPED, xl.SMAX)
        assert raw[4] == S_wc - 1 and sh.last_specH > 0.0
        sh.extend = True
        out = {t: _kernel(torch, sh, t, xl.SMAX) for t in (SHIPPED, UPPER, COMPILER)}
        for t in (UPPER, COMPILER):
            _assert_same(torch, out[t], out[SHIPPED], "extension, tune %d against the default" % t)
        assert out[SHIPPED][3] == klive
        v_raw, v_ext = raw[1].cpu().numpy(), out[SHIPPED][1].cpu().numpy()
        changed = v_ext != v_raw
        assert 1 <= changed.sum() <= 64
        np.testing.assert_array_equal(v_ext[changed], vara[changed])
    finally:
        os.environ.pop("EAGLE_HIP_EXT_CAP")
        _tune(sh, SHIPPED)
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)
        sh.ws = None


def test_second_block_of_a_streamed_scan_keeps_the_count():
    """eagle_dev_vara_i8_prepare_part: part 1 once, then part 2 + the kernel for two marker blocks of 512 through one workspace.  n = 600:
    klive = 5 of 6 -- a count that part 2 zeroed would cut tiles 0 and 1 down to their floor and lose products."""
    import torch
    from eagleeverything_amd.sharded import DeviceShard
    n, S, Lb = 600, 4, 512
    case, a, vara, klive = _designed(n, S, "dense")
    sh = DeviceShard(n, L)
    sh.Mt8[:L, :n] = torch.from_numpy(case["Mt8"].copy()).to(sh.dev)
    sh.mode, sh.nslices, sh.packed = 1, S, False
    sh.set_W(np.ldexp(case["X"].astype(np.float64), case["log2u"]), case["ahat"])
    sh.scan_operands()
    q_res, v_res, _, kl_res, _, _ = _kernel(torch, sh, SHIPPED, S)
    assert kl_res == klive == 5 and sh.Lp == 2 * Lb
    Ms, cs = sh.shifted_image()
    part = sh.L.eagle_dev_vara_i8_prepare_part
    part.restype = C.c_int
    part.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    ws = torch.full((int(sh.L.eagle_vara_i8_workspace_bytes(sh.np_, Lb, S)),), POISON, dtype=torch.uint8, device=sh.dev)
    a_b = torch.zeros(Lb, dtype=torch.float64, device=sh.dev)
    v_b = torch.zeros(Lb, dtype=torch.float64, device=sh.dev)
    sh._check(part(sh.ctx, sh.Mt8.data_ptr(), Lb, sh.np_, sh.np_, sh.Wu.data_ptr(), S, ws.data_ptr(), None, None, sh._stream(), 1))
    for b in range(2):
        rows = slice(b * Lb, (b + 1) * Lb)
        sh._check(part(sh.ctx, sh.Mt8[rows].data_ptr(), Lb, sh.np_, sh.np_, sh.Wu.data_ptr(), S, ws.data_ptr(), sh.v.data_ptr(), a_b.data_ptr(),
                       sh._stream(), 2))
        sh._check(sh.L.eagle_dev_vara_i8_mfma_shifted(sh.ctx, Ms[rows].data_ptr(), cs[rows].data_ptr(), Lb, sh.np_, sh.np_, S, ws.data_ptr(),
                                                      v_b.data_ptr(), None, sh._stream()))
        torch.cuda.synchronize()
        assert int(ws[128:132].view(torch.int32).item()) == klive, "block %d" % b
        q_b = ws[256:256 + 8 * S * Lb].view(torch.int64).view(S, Lb)
        assert torch.equal(q_b, q_res.view(S, sh.Lp)[:, rows]), "q of block %d" % b
        assert torch.equal(v_b, sh.vara[rows]), "vara of block %d" % b
        live = min(L, (b + 1) * Lb) - b * Lb
        np.testing.assert_array_equal(v_b[:live].cpu().numpy(), vara[b * Lb:b * Lb + live])
        np.testing.assert_array_equal(a_b[:live].cpu().numpy(), a[b * Lb:b * Lb + live])
