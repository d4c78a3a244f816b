"""The spectral last-digit path of the digit-slice scan against an exact integer truth (tests/exact_lastdigit.py, pinned on the CPU by
tests/test_lastdigit_exact_host.py).

The default path of the scan takes one digit off under the spectral bound (csrc/eagle_i8mfma.hip: k_slice_w's symmetric last-digit
image, the fused k_gram_rowabs_i8<true> epilogue, k_gram_hi_settle, k_spectral_decide, the scan on S_sliced - 1 digits,
eagle_dev_vara_i8_extend).  On operands whose last digit is chosen and whose diagonal puts the digit rule into a chosen state, everything
that path leaves behind is an integer the host can restate, and every comparison below is an equality -- but for the bound H itself, which
carries the library's round-up factors: H_host <= specH <= H_host (1 + 1e-12), with max row sum < 1e10 so that one unit in the largest row
sum moves H by more than that allowance.

(a) the image Ds, E_hi, the row sums of |E_hi E_hi| and the header in three states of the rule at four shapes; (b) Gram entries planted on
hi = 127 / -128 (and 128 / -129: no level-2 bound) and lo = -2^(s-1) / 2^(s-1) - 1, inside diagonal tiles and in a mirrored tile; (c) the
largest row sum planted on every row next to a block, wave-half and tile edge; (d) the scan on one digit fewer: raw value = truth minus
exactly the last digit's term, inside specH q2 with no additive term, the extension giving the flagged markers the truth bit for bit
(S_sliced = 4), taking its flags back without a spare slot (S_sliced = 5) where the certificate rescues them, and level 1 alone at
S_sliced = 6."""
import ctypes as C

import numpy as np
import pytest

import exact_lastdigit as xl
import exact_scan as ex

pytestmark = pytest.mark.gpu
POISON = 0xA5


@pytest.fixture(scope="module")
def api():
    from eagleeverything_amd import rcpp_api
    assert rcpp_api.device_info()["arch"].startswith("gfx950")
    yield rcpp_api
    rcpp_api.close_all()


def _shard(case, api, packed=True):
    import torch
    from eagleeverything_amd.sharded import DeviceShard
    sh = DeviceShard(case["n"], case["L"])
    assert sh.np_ == case["n_pad"]
    sh.Mt8[:case["L"], :case["n"]] = torch.from_numpy(case["Mt8"].copy()).to(sh.dev)
    sh.set_operands(case["S"], case["V"], case["ahat"])
    sh.L.eagle_dev_set_spectral(sh.ctx, 1)                               # the default path: one digit off under the spectral bound
    sh._check(sh.L.eagle_set_scan_budget(sh.ctx, 0.0))                   # the default policy: 1e-7 first, then 5e-7
    sh.mode, sh.nslices, sh.packed = 1, 0, packed
    return torch, sh


def _prepare(torch, sh):
    """prepare on a workspace poisoned with 0xA5 -> (header dict, {slot: n_pad x n_pad int8}, n_pad uint64 of the row-sum area)."""
    ws = sh._ws()
    ws.fill_(POISON)
    sh.scan_operands()
    sh.vara_prepare()
    torch.cuda.synchronize()
    hdr = xl.decode_header(ws[:256].cpu().numpy())
    nslots = C.c_int(0)
    n2 = sh.np_ * sh.np_
    slots = {}
    for k in (xl.SMAX - 2, xl.SMAX - 1):
        off = int(sh.L.eagle_vara_i8_ws_slot_offset(sh.np_, sh.Lp, 0, k, C.byref(nslots)))
        slots[k] = ws[off:off + n2].cpu().numpy().view(np.int8).reshape(sh.np_, sh.np_).copy()
    assert nslots.value == xl.SMAX
    off = int(sh.L.eagle_vara_i8_ws_rowsum_offset(sh.np_, sh.Lp, 0))
    rows = ws[off:off + 8 * sh.np_].cpu().numpy().view(np.uint64).copy()
    return hdr, slots, rows


def _first_diff(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return None if bad.size == 0 else (tuple(int(x) for x in bad[0]), int(bad.shape[0]))


def _assert_prepared(case, hdr, slots, rows, what):
    """Image, E_hi, row sums and header against the restatement; the bound inside the allowance of the round-up factors."""
    R, n = case["R"], case["n"]
    level, H_host, b, ran2 = case["decision"]
    want = xl.expected_header(case)
    got = {k: hdr[k] for k in want}
    print(what, "header", got, "specH %r specH1 %r host H1 %r H2 %r" % (hdr["specH"], hdr["specH1"], case["H1"], case["H2"]))
    Ds = slots[xl.SMAX - 1]
    bad = _first_diff(Ds, R["Ds"].astype(np.int8))
    assert bad is None, "%s: last-digit image, first wrong entry %r of %d" % ((what,) + bad)
    assert np.array_equal(Ds, Ds.T) and not Ds.diagonal().any() and not Ds[n:].any() and not Ds[:, n:].any()
    assert got == want, (what, got, want)
    assert hdr["sumdiag"] == float(case["sumdiag"]) and hdr["wErr"] == 0.0
    if ran2:
        bad = _first_diff(slots[xl.SMAX - 2], R["hi8"])
        assert bad is None, "%s: E_hi, first wrong entry %r of %d" % ((what,) + bad)
        bad = _first_diff(rows, R["rs2"].astype(np.uint64))
        assert bad is None, "%s: row sums of |E_hi E_hi|, first wrong row %r of %d" % ((what,) + bad)
    assert R["rs1"].max() < 1e10
    if level:
        assert H_host <= hdr["specH"] <= H_host * (1 + 1e-12), (what, H_host, hdr["specH"])
    else:
        assert hdr["specH"] == 0.0, (what, hdr["specH"])
    if ran2:   # level 1's bound, kept while level 2 was tried
        assert case["H1"] <= hdr["specH1"] <= case["H1"] * (1 + 1e-12), (what, case["H1"], hdr["specH1"])
    else:
        assert hdr["specH1"] == 0.0


@pytest.mark.parametrize("n", xl.SHAPES)
def test_image_gram_and_header_are_the_integer_truth(n, api):
    """(a): n -> n_pad = 200 -> 256 (one tile pair, diagonal only), 300 -> 512 (one mirrored pair, 212 padding rows), 700 -> 768 (three row
    panels), 1003 -> 1024 (10 pairs: the XCD remap of the pair list has two per XCD), each in the states `level 2 takes the digit`, `level 2
    runs, level 1's bound passes at the default budget` and `nobody passes`."""
    for state in xl.PREP_STATES:
        case = xl.prep_case(n, state)
        xl.assert_state(case)
        torch, sh = _shard(case, api)
        hdr, slots, rows = _prepare(torch, sh)
        _assert_prepared(case, hdr, slots, rows, "n=%d %s" % (n, state))
        assert (hdr["level"], hdr["S"]) == {"l2": (2, 3), "l1_default": (1, 3), "none": (0, 4)}[state]
        del sh


@pytest.mark.parametrize("n", [300, 700])
def test_planted_gram_entries_at_the_int8_and_rounding_edges(n, api):
    """(b): hi = 127 / -128 with lo = -2^(s-1) / 2^(s-1) - 1 below and above the diagonal of a diagonal tile and in a mirrored tile; then
    hi = 128 / -129: hi_overflow, no level-2 bound, level 1's bound at the default budget where it passes, else nothing taken off."""
    case = xl.planted_case(n, "l2")
    xl.assert_state(case)
    torch, sh = _shard(case, api)
    hdr, slots, rows = _prepare(torch, sh)
    _assert_prepared(case, hdr, slots, rows, "n=%d planted edges" % n)
    assert (hdr["level"], hdr["hi_overflow"]) == (2, 0)
    E = slots[xl.SMAX - 2]
    for name, pairs in case["planted"].items():
        for j, k in pairs:
            assert E[j, k] == E[k, j] == (127 if name.startswith("hi=127") else -128), (name, j, k, E[j, k], E[k, j])
    del sh
    for plant in ("overflow", "overflow+", "overflow-"):                  # both planted, then each side alone: either raises the flag
        case = xl.planted_case(n, "ovf_l1", plant)
        xl.assert_state(case)
        torch, sh = _shard(case, api)
        hdr, slots, rows = _prepare(torch, sh)
        _assert_prepared(case, hdr, slots, rows, "n=%d %s, level 1 at the default budget" % (n, plant))
        assert (hdr["hi_overflow"], hdr["level"], hdr["budget"], hdr["S"], hdr["S_sliced"]) == (1, 1, xl.BUDGET, 3, 4)
        assert hdr["specH"] == hdr["specH1"] > 0.0
        del sh
    case = xl.planted_case(n, "ovf_none")
    xl.assert_state(case)
    torch, sh = _shard(case, api)
    hdr, slots, rows = _prepare(torch, sh)
    _assert_prepared(case, hdr, slots, rows, "n=%d overflow, nobody passes" % n)
    assert (hdr["hi_overflow"], hdr["level"], hdr["specH"], hdr["S"], hdr["S_sliced"]) == (1, 0, 0.0, 4, 4)


def test_largest_row_sum_on_every_row_next_to_an_edge(api):
    """(c): the bound follows the planted maximum wherever it lies: both 128-row wave halves, every 32-row MFMA block edge, the tile edge
    at 255 / 256 and the last live row 299, which the column sums of the off-diagonal tile carry."""
    sh = None
    for r in xl.LOUD_ROWS:
        case = xl.loud_case(r)
        xl.assert_state(case)
        if sh is None:
            torch, sh = _shard(case, api)
        else:
            sh.set_operands(case["S"], case["V"], case["ahat"])
        hdr, slots, rows = _prepare(torch, sh)
        assert int(np.argmax(case["R"]["rs1"])) == r
        _assert_prepared(case, hdr, slots, rows, "loud row %d" % r)
        assert (hdr["level"], hdr["budget"]) == (1, xl.TIGHT)


def _run(torch, sh, L):
    sh.scan()
    torch.cuda.synchronize()
    t, i0, _ = sh.best()
    return sh.a[:L].cpu().numpy().copy(), sh.vara[:L].cpu().numpy().copy(), i0 + 1, t


@pytest.mark.parametrize("name", sorted(xl.SCAN_CASES))
def test_scan_on_one_digit_fewer_is_the_truth_minus_the_last_digit(name, api):
    """(d): the automatic path, spectral bound on.  All S_wc digits hold W exactly, so the scan on S_wc - 1 of them misses exactly
    unit x sum_{j<k} m'_j m'_k d_jk -- an equality -- and that miss is inside specH q2 with no additive term."""
    n, L, S_wc, state, packed = xl.SCAN_CASES[name]
    case = xl.scan_case(name)
    xl.assert_state(case)
    a, vara, units = ex.scan_truth(case)
    best = ex.argmax_truth(a, units, case)
    torch, sh = _shard(case, api, packed)
    try:
        sh.certified, sh.extend = False, False
        a_raw, raw, _, _ = _run(torch, sh, L)
        S_used = sh.vara_i8_info()[0]
        hdr = xl.decode_header(sh.ws[:256].cpu().numpy())
        assert (S_used, sh.last_sliced, sh.last_e, sh.last_level) == (S_wc - 1, S_wc, xl.E_SCALE, case["decision"][0]), hdr
        H_host = case["decision"][1]
        assert H_host <= sh.last_specH <= H_host * (1 + 1e-12) and sh.last_budget == case["decision"][2]
        np.testing.assert_array_equal(a_raw, a)
        c = sh.cshift[:L].cpu().numpy().astype(np.int64)
        np.testing.assert_array_equal(c, xl.recentre(case["Mt8"]))
        miss, q2, l1 = xl.lastdigit_miss_units(case, c)
        l1q2 = sh.l1[:L].cpu().numpy().astype(np.int64)
        np.testing.assert_array_equal(l1q2[:, 0], l1)
        np.testing.assert_array_equal(l1q2[:, 1], q2)
        want = np.ldexp((units - miss).astype(np.float64), case["log2u"])
        bad = np.flatnonzero(raw != want)
        assert bad.size == 0, "%s: raw value of %d markers, first %d: %r, truth minus the last digit %r" % (name, bad.size, bad[0], raw[bad[0]], want[bad[0]])
        err = np.abs(raw - vara)                                         # exact: both are multiples of u below 2^53 u
        bound = sh.last_specH * q2
        worst = int(np.argmax(err - bound))
        assert np.all(err <= bound), (worst, err[worst], bound[worst])
        assert np.count_nonzero(err) >= L // 4
        adv = np.array(case["adv_rows"])
        print("%s: largest |err| / (specH q2): adversarial %.4f, any marker %.4f" % (name, (err[adv] / bound[adv]).max(), (err[bound > 0] / bound[bound > 0]).max()))
        if S_wc == 6:                                                    # level 1 alone: the fused kernel's level-2 side stayed off
            assert (hdr["level"], hdr["lo_sumsq"], hdr["maxdiag"], hdr["hi_overflow"], hdr["specH1"]) == (1, 0, 0, 0, 0.0)
            return
        flag, ratio = xl.extension_flags(raw, l1, q2, sh.last_specH, sh.last_budget, xl.E_SCALE, S_used)
        qr = np.array(case["quiet_rows"])
        assert 1 <= flag[qr].sum() <= 64 and not np.any((ratio > 0.99) & (ratio < 1.01)) and np.all(err[flag] > 0)
        sh.extend = True
        _, v_ext, _, _ = _run(torch, sh, L)
        assert sh.vara_i8_info()[0] == S_wc - 1 and sh.last_specH > 0.0
        if S_wc == 4:     # a spare slot: the flagged markers get the dropped digit back and carry the truth, everyone else the raw value
            np.testing.assert_array_equal(v_ext[flag], vara[flag])
            np.testing.assert_array_equal(v_ext[~flag], raw[~flag])
        else:             # S_sliced = 5: no spare slot, the flags are taken back and nobody changes ...
            np.testing.assert_array_equal(v_ext, raw)
        # ... certified: the truth or the raw value per marker, the flagged ones the truth, the rational arg-max selected
        sh.certified = True
        a1, cert, i1, t1 = _run(torch, sh, L)
        info = sh.certificate()
        assert info["overflow"] == 0, info
        np.testing.assert_array_equal(a1, a)
        exact = cert == vara
        assert np.all(exact | (cert == raw))
        assert np.all(exact[flag]), np.flatnonzero(flag & ~exact)
        assert i1 == best[0] and exact[i1 - 1] and ex.ulp_distance(t1, float(best[1])) <= 2
        _run(torch, sh, L)
        assert sh.vara_i8_info()[0] == S_wc - 1 and sh.last_specH > 0.0    # no fallback: the digit stays off on the next scan
    finally:
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)
