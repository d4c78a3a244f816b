"""The scan kernels against an exact integer truth (tests/exact_scan.py, pinned on the CPU by tests/test_scan_exact_host.py).

With S = s I, a symmetric V of dyadic entries and an integer a_hat every product of W = S (V S), every a_i and every vara_i is an
integer times a power of two that fp64 holds, so every summation order -- the fp64 MFMA kernel, the int8 digit-slice kernel with its
prepare, shift and finish steps, the certificate's re-evaluation, a streamed or sharded panel -- must return the same bits: all
comparisons below are equalities.  One wrong element of W (a pair dropped on a tile diagonal, a pad row read as data, a digit that
carries wrongly at -128 / +127) moves a typical vara by 1e-6 of its value, which the tolerance tests of this suite let through; here
the probe markers e_j + e_k, e_j - e_k, e_j name it: vara(e_j + e_k) - vara(e_j - e_k) = 4 W_jk, vara(e_j) = W_jj.

Digits: the off-diagonal entries are u x with the edge patterns d2 65536 + d1 256 + d0, d in {-128, -127, -1, 0, 1, 127}, on both sides
of every 256 / 384 boundary, and one entry 2^22 - 1 fixes the scale exponent e = 23, so that with S slices the unit of the last digit of
the folded entries 2 W_jk is 2^(25 - 8 S) = 2 u for u = 2^(24 - 8 S): x itself is what gets cut into digits.  Seven slices span 56 bits,
more than a double: there u = 2^-24 (exact_scan.LOG2U_OF_SLICES says why), patterns on digits 1..3.  e and the slice count are read
back and asserted, never assumed."""
import functools

import numpy as np
import pytest

import exact_scan as ex
from eagleeverything_amd import synth

pytestmark = pytest.mark.gpu
NA = np.nan
# n: 1, 2, around 256 and 384 (the tile heights of the two digit kernels), several tiles, the last row of a 1,024 pad; L: one marker, a
# ragged tile and a half, 1,000
SHAPES = [(1, 1), (1, 1000), (2, 129), (255, 257), (256, 129), (257, 1), (257, 1000), (383, 257), (385, 1), (385, 1000), (640, 129), (1003, 1),
          (1003, 257), (1003, 1000)]
FORCED = [(4, n, L) for n, L in SHAPES] + [(S, n, L) for S in (3, 5, 7) for n, L in ((2, 129), (257, 1000), (385, 1), (1003, 1000))]


@pytest.fixture(scope="module")
def api():
    from eagleeverything_amd import rcpp_api
    assert rcpp_api.device_info()["arch"].startswith("gfx950")
    yield rcpp_api
    rcpp_api.close_all()


@functools.lru_cache(maxsize=None)
def _case(n, L, log2u, s=1, small=False):
    """(operands, a, vara, vara in units of s^2 u, (1-based arg-max, its tsq as a Fraction)): built and bounded once, never written to."""
    case = ex.build_case(n, L, log2u=log2u, s=s, small=small)
    ex.check_exact(case)                                                 # Python ints: every partial sum is a double, before the device is asked
    a, vara, units = ex.scan_truth(case)
    for arr in (case["X"], a, vara, units):
        arr.setflags(write=False)
    return case, a, vara, units, ex.argmax_truth(a, units, case)


def _assert_scan(case, a_dev, v_dev, a, vara, what):
    """a and vara bit for bit; a wrong element of W names itself through its probe markers first."""
    a_dev, v_dev = np.ravel(a_dev), np.ravel(v_dev)
    u = 2.0 ** case["log2u"] * case["s"] ** 2
    for (j, k), (rp, rm, r1) in case["probes"].items():
        assert v_dev[r1] == case["X"][j, j] * u, "%s: W[%d][%d] = %r, truth %r" % (what, j, j, v_dev[r1], case["X"][j, j] * u)
        assert v_dev[rp] - v_dev[rm] == 4.0 * case["X"][j, k] * u, \
            "%s: W[%d][%d] = %r, truth %r" % (what, j, k, (v_dev[rp] - v_dev[rm]) / 4.0, case["X"][j, k] * u)
    bad = np.flatnonzero(v_dev != vara)
    assert bad.size == 0, "%s: vara of %d markers, first %d: %r, truth %r" % (what, bad.size, bad[0], v_dev[bad[0]], vara[bad[0]])
    np.testing.assert_array_equal(a_dev, a, err_msg=what)
    if case["zero"] is not None:                                         # (the all +1 / all -1 markers, the extremes of the shift, are rows of `vara`)
        assert a_dev[case["zero"]] == 0.0 and v_dev[case["zero"]] == 0.0 and vara[case["plus"]] == vara[case["minus"]] > 0.0


def _assert_argmax(case, best, idx1, tsqmax, what):
    """First index of the exact rational maximum over the non-NaN markers; the reported maximum within 2 ulp of it (one rounding is in the
    division, and include/eagle_hip.h fixes no more than that)."""
    idx, mx = best
    assert idx1 == idx, (what, idx1, idx)
    if idx == 0:
        assert np.isnan(tsqmax), what
        return
    assert ex.ulp_distance(tsqmax, float(mx)) <= 2, (what, tsqmax, float(mx))
    if case["dup"] is not None and case["n"] >= 255:
        assert idx == case["dup"][0] + 1, "construction: the duplicated pair holds the maximum and its first index wins"


def _shard(case, api):
    import torch
    from eagleeverything_amd.sharded import DeviceShard
    sh = DeviceShard(case["n"], case["L"])
    sh.Mt8[:case["L"], :case["n"]] = torch.from_numpy(case["Mt8"].copy()).to(sh.dev)
    sh.set_operands(case["S"], case["V"], case["ahat"])
    sh.L.eagle_dev_set_spectral(sh.ctx, 0)                               # no digit is taken off under the spectral bound
    return torch, sh


def _run(torch, sh, L):
    sh.scan()
    torch.cuda.synchronize()
    t, i0, _ = sh.best()
    return sh.a[:L].cpu().numpy().copy(), sh.vara[:L].cpu().numpy().copy(), i0 + 1, t


def _digits(sh):
    S_used = sh.vara_i8_info()[0]
    return S_used, sh.last_e


def _digit_scan_is_exact(torch, sh, case, a, vara, best, a0, what):
    """Raw digit values (certificate off), then certified: both the truth, a the fp64 scan's, the exact arg-max."""
    L = case["L"]
    sh.mode = 1
    sh.certified = False
    a_raw, v_raw, _, _ = _run(torch, sh, L)
    _assert_scan(case, a_raw, v_raw, a, vara, what + " raw digits")
    sh.certified = True
    a1, v1, i1, t1 = _run(torch, sh, L)
    _assert_scan(case, a1, v1, a, vara, what + " certified")
    assert sh.certificate()["overflow"] == 0
    np.testing.assert_array_equal(a1, a0)
    _assert_argmax(case, best, i1, t1, what)


@pytest.mark.parametrize("n,L", SHAPES)
def test_fp64_scan_reference_shaped_call_is_the_integer_truth(n, L, api, tmp_path):
    """(a), (e): k_gemv_mfma, k_vara_f64d, k_tsq and the arg-max through calculate_a_and_vara_rcpp, scan mode 0."""
    case, a, vara, units, best = _case(n, L, -8)
    geno = synth.write_geno_pair(str(tmp_path), case["Mt8"])
    try:
        api.set_scan_mode(0)
        res = api.calculate_a_and_vara_rcpp(geno["asciifileMt"], NA, case["S"], case["V"], 8.0, (L, n), case["ahat"])
        idx1, tsqmax, _ = api.last_scan_argmax()
    finally:
        api.set_scan_mode(1)
        api.drop_cache()
    _assert_scan(case, res["a"], res["vara"], a, vara, "mode 0 n=%d L=%d" % (n, L))
    _assert_argmax(case, best, idx1, tsqmax, "mode 0")


@pytest.mark.parametrize("S,n,L", FORCED)
def test_digit_slice_scan_forced_slices_is_the_integer_truth(S, n, L, api):
    """(b), (e): k_vara_i8p with the digit prepare, the marker shift, the finish and the certificate on S forced slices whose digits hold
    the operands exactly -- the image is exact, so the kernel has nothing to lose."""
    case, a, vara, units, best = _case(n, L, ex.LOG2U_OF_SLICES[S])
    torch, sh = _shard(case, api)
    try:
        sh.mode = 0
        a0, v0, i0, t0 = _run(torch, sh, L)
        _assert_scan(case, a0, v0, a, vara, "device mode 0")
        _assert_argmax(case, best, i0, t0, "device mode 0")
        sh.mode, sh.nslices = 1, S
        sh.certified = False
        sh.scan()
        torch.cuda.synchronize()
        S_used, e = _digits(sh)
        if n > 1:   # precondition of the construction, a failure and not a skip: S digits on the scale of the planted 2^22 - 1, nothing taken off
            assert (S_used, sh.last_sliced, e, sh.last_specH) == (S, S, 23, 0.0), (S_used, sh.last_sliced, e, sh.last_specH)
            assert 2.0 ** (e + 2 - 8 * S_used) <= 2.0 * 2.0 ** case["log2u"]   # unit of the last digit <= the step 2 u of the folded entries
        else:
            assert S_used == 1                                           # no off-diagonal entry at all
        _digit_scan_is_exact(torch, sh, case, a, vara, best, a0, "S=%d n=%d L=%d" % (S, n, L))
    finally:
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)


@pytest.mark.parametrize("n,L", [(2, 129), (257, 1000), (640, 129), (1003, 1000)])
def test_digit_slice_scan_automatic_slices_is_the_integer_truth(n, L, api):
    """(c): the library's own digit count.  u = 2^-6; the count it chooses must put the unit of the last digit at or below u (asserted from
    the read-back), and then the same equalities hold."""
    case, a, vara, units, best = _case(n, L, -6)
    torch, sh = _shard(case, api)
    try:
        sh.mode = 0
        a0, v0, _, _ = _run(torch, sh, L)
        _assert_scan(case, a0, v0, a, vara, "device mode 0")
        sh.mode, sh.nslices = 1, 0
        sh.certified = False
        sh.scan()
        torch.cuda.synchronize()
        S_used, e = _digits(sh)
        assert e == 23 and sh.last_sliced == S_used and sh.last_specH == 0.0, (e, S_used, sh.last_sliced, sh.last_specH)
        assert 2.0 ** (e + 2 - 8 * S_used) <= 2.0 ** case["log2u"], "precondition: unit 2^%d above u" % (e + 2 - 8 * S_used)
        _digit_scan_is_exact(torch, sh, case, a, vara, best, a0, "auto S=%d n=%d L=%d" % (S_used, n, L))
    finally:
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)


@pytest.mark.parametrize("n,L", [(385, 1000), (1003, 1000)])
def test_streamed_and_sharded_panels_are_the_integer_truth(n, L, api, tmp_path, monkeypatch):
    """(d): the reference-shaped digit-slice call (four forced slices) resident, streamed in 256-marker blocks and on two sub-contexts of
    the card: each the truth, not just each other."""
    case, a, vara, units, best = _case(n, L, -8)
    geno = synth.write_geno_pair(str(tmp_path), case["Mt8"])
    call = lambda dev: api.calculate_a_and_vara_rcpp(geno["asciifileMt"], NA, case["S"], case["V"], 8.0, (L, n), case["ahat"], device=dev)
    np_ = (n + 255) // 256 * 256
    try:
        api.set_scan_mode(1)
        api.set_scan_slices(4)
        res = call(0)
        assert api.last_scan_digits()[:2] == (4, 4)
        _assert_scan(case, res["a"], res["vara"], a, vara, "resident")
        _assert_argmax(case, best, *api.last_scan_argmax()[:2], "resident")
        api.drop_cache()
        monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "%.6f" % (2.0 * 256 * np_ / 1e9))
        res = call(0)
        assert api.last_stream_stats()["chunks"] > 1
        _assert_scan(case, res["a"], res["vara"], a, vara, "streamed")
        _assert_argmax(case, best, *api.last_scan_argmax()[:2], "streamed")
        monkeypatch.delenv("EAGLE_HIP_MAX_RESIDENT_GB")
        api.drop_cache()
        dev = (0, 0)
        api.set_scan_mode(1, device=dev)
        api.set_scan_slices(4, device=dev)
        res = call(dev)
        _assert_scan(case, res["a"], res["vara"], a, vara, "two sub-contexts")
        _assert_argmax(case, best, *api.last_scan_argmax(device=dev)[:2], "two sub-contexts")
    finally:
        monkeypatch.delenv("EAGLE_HIP_MAX_RESIDENT_GB", raising=False)
        api.set_scan_slices(0)
        api.drop_cache()
        if (0, 0) in api._ctx:
            api.set_scan_slices(0, device=(0, 0))
            api.drop_cache(device=(0, 0))


@pytest.mark.parametrize("n", [640, 1003])
def test_int8_w_engine_is_exact_on_integer_operands(n, api):
    """(f): W = S (V S) on the int8 engine with S = 2 I and small-integer V (|x| <= 3).  S has no off-diagonal part, so both digit-slice
    products of the engine vanish and W is made of its exact diagonal terms: the folded image must be 4 V folded, bit for bit, and the
    digit-slice scan on it the truth."""
    L = 257
    case, a, vara, units, best = _case(n, L, 0, 2, True)
    torch, sh = _shard(case, api)
    try:
        sh.mode = 0
        a0, v0, _, _ = _run(torch, sh, L)
        _assert_scan(case, a0, v0, a, vara, "device mode 0")
        sh.mode, sh.w_mode, sh.nslices = 1, 2, 3
        sh.scan_operands()
        torch.cuda.synchronize()
        info = sh.w_info()
        assert info["int8"] == 1, info
        fold = 4.0 * ex.fold_units(case).astype(np.float64)
        np.testing.assert_array_equal(sh.Wu[:n, :n].cpu().numpy(), fold)
        assert float(sh.Wu[n:, :].abs().max()) == 0.0 and float(sh.Wu[:, n:].abs().max()) == 0.0
        np.testing.assert_array_equal(sh.v[:n].cpu().numpy(), 2.0 * case["ahat"])
        _digit_scan_is_exact(torch, sh, case, a, vara, best, a0, "int8 W n=%d" % n)
        assert sh.w_info()["int8"] == 1
    finally:
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)


@pytest.mark.parametrize("n,L", [(257, 1000), (1003, 1000)])
def test_digit_bound_without_slack_one_slice_short(n, L, api):
    """(g): three slices on operands that need four (u = 2^-8).  Every other term of the finish step is still exact, so raw - truth is the
    truncation of W alone: inside 0.5 l1^2 2^(e+1-8S) (1 + 2^-8) with no additive term -- and, sharper, exactly
    -sum_{j<k} m'_j m'_k r_jk for the residuals r of the host restatement and the re-centring c the shard reports.  Certified: inside
    1.8 x the budget in force; the probe markers are flagged by their own bound and come back exact."""
    S = 3
    case, a, vara, units, best = _case(n, L, -8)
    M = case["Mt8"].astype(np.int64)
    R = ex.digit_residual_units(case, S, 23)
    cnt = np.stack([(M == g).sum(axis=1) for g in (-1, 0, 1)], axis=1)
    c_host = np.where(cnt[:, 1] >= np.maximum(cnt[:, 0], cnt[:, 2]), 0, np.where(cnt[:, 0] >= cnt[:, 2], -1, 1))
    Mh = M - c_host[:, None]
    resid_host = (ex._exact_matmul(Mh, R) * Mh).sum(axis=1)
    assert np.count_nonzero(resid_host) >= L // 4, "construction: an all-zero error would satisfy the bound vacuously"
    torch, sh = _shard(case, api)
    try:
        sh.mode, sh.nslices = 1, S
        sh.certified = False
        a_raw, raw, _, _ = _run(torch, sh, L)
        S_used, e = _digits(sh)
        assert (S_used, e, sh.last_specH) == (S, 23, 0.0)
        np.testing.assert_array_equal(a_raw, a)
        l1 = sh.l1[:L, 0].cpu().numpy().astype(np.float64)
        bound = 0.5 * l1 * l1 * 2.0 ** (e + 1 - 8 * S) * (1 + 2.0 ** -8)
        err = np.abs(raw - vara)                                         # exact: both are multiples of u below 2^53 u
        worst = int(np.argmax(err - bound))
        assert np.all(err <= bound), (worst, err[worst], bound[worst])
        assert np.count_nonzero(err) >= L // 4
        c = sh.cshift[:L].cpu().numpy().astype(np.int64)
        Ms = M - c[:, None]
        resid = (ex._exact_matmul(Ms, R) * Ms).sum(axis=1)
        np.testing.assert_array_equal(raw, np.ldexp((units - resid).astype(np.float64), case["log2u"]))
        sh.certified = True
        _, cert, i1, t1 = _run(torch, sh, L)
        info = sh.certificate()
        assert info["overflow"] == 0
        sh.vara_i8_info()
        exact = cert == vara
        assert np.all(np.abs(cert - vara)[~exact] <= 1.8 * sh.last_budget * np.abs(cert)[~exact])
        assert np.all(exact | (cert == raw))                             # re-evaluated in fp64 (the truth) or left as the digits gave it
        # the probes: zero is their commonest genotype, the shift centres such a marker on its commoner homozygote, l1 ~ n: their own bound is
        # far above the threshold, they are flagged and come back as the truth
        rows = np.array([r for t in case["probes"].values() for r in t])
        assert np.all(bound[rows] > 1.8 * sh.last_budget * np.abs(raw[rows])) and np.all(exact[rows]), rows[~exact[rows]]
        assert exact[i1 - 1] and i1 == best[0] and ex.ulp_distance(t1, float(best[1])) <= 2   # the selected marker carries its fp64 value
    finally:
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)
