"""tests/exact_lastdigit.py pinned on the CPU: the numpy restatement of the last digit's Gram product against a plain Python-int loop,
and every precondition of tests/test_gpu_lastdigit_exact.py -- the state each case reaches under the restated digit rule, the planted
values, the exactness bound of tests/exact_scan.py, the identity the scan test relies on and its non-vacuity counts -- so that nobody finds
out on the GPU that a case is vacuous."""
import numpy as np
import pytest

import exact_lastdigit as xl
import exact_scan as ex


def test_restatement_equals_a_python_int_triple_loop():
    n, n_pad = 37, 256
    rng = np.random.default_rng(37)
    d = np.triu(rng.integers(-128, 128, size=(n, n)), 1)
    d[0, 1:] = 127                                                        # large entries of G: both signs of hi, some outside int8
    d[1, 2:] = -128
    d[1, 2::2] = 127
    R, P = xl.restate(d, n_pad), xl.restate_python(d, n_pad)
    s = R["shift"]
    assert s == xl.gram_shift(256) == 13
    for key in ("Ds", "G", "hi"):
        assert np.array_equal(R[key][:n, :n], np.array(P[key], dtype=np.int64)), key
        assert not R[key][n:].any() and not R[key][:, n:].any()
    for key in ("rs1", "rs2"):
        assert R[key][:n].tolist() == P[key] and not R[key][n:].any(), key
    for key in ("lo_sumsq", "maxdiag", "overflow"):
        assert R[key] == P[key], key
    assert np.array_equal(R["Ds"], R["Ds"].T) and not np.diag(R["Ds"]).any()
    assert R["lo"].min() >= -(1 << (s - 1)) and R["lo"].max() < (1 << (s - 1))
    assert np.array_equal((R["hi"] << s) + R["lo"], R["E"]) and not np.diag(R["E"]).any()
    # a product of 36 terms of 128 x 127 does not leave int8 at s = 13: the wrapped image is the plain one here ...
    assert R["overflow"] == 0 and np.array_equal(R["hi8"], R["hi"])
    # ... and where it does, the image wraps as a byte store does
    d2 = np.zeros((300, 300), dtype=np.int64)
    d2[0, 2:82] = 127
    d2[1, 2:82] = 127
    R2 = xl.restate(d2, 512)
    assert R2["overflow"] == 1 and R2["hi"][0, 1] == (80 * 127 * 127 + 4096) >> 13 == 158 and R2["hi8"][0, 1] == 158 - 256


def test_rounding_of_e_hi_at_the_half():
    """hi = floor((v + 2^(s-1)) / 2^s): v = 2^(s-1) (mod 2^s) goes up, one below stays; lo in [-2^(s-1), 2^(s-1))."""
    for s in (13, 14):
        T = xl.edge_targets(s, "edge")
        half = 1 << (s - 1)
        got = {k: ((v + half) >> s, v - (((v + half) >> s) << s)) for k, v in T.items()}
        assert got == {"hi=127,lo=-half": (127, -half), "hi=127,lo=half-1": (127, half - 1), "hi=-128,lo=half-1": (-128, half - 1),
                       "hi=-128,lo=-half": (-128, -half)}
        assert {k: (v + half) >> s for k, v in xl.edge_targets(s, "overflow").items()} == {"hi=128": 128, "hi=-129": -129}
        assert list(xl.edge_targets(s, "overflow+")) == ["hi=128"] and list(xl.edge_targets(s, "overflow-")) == ["hi=-129"]


def test_decoder_reads_the_header_layout():
    raw = np.zeros(256, dtype=np.uint8)
    raw[8:12] = np.frombuffer(np.int32(3).tobytes(), dtype=np.uint8)
    raw[72:80] = np.frombuffer(np.uint64(2 ** 40 + 5).tobytes(), dtype=np.uint8)
    raw[92:96] = np.frombuffer(np.int32(2).tobytes(), dtype=np.uint8)
    raw[56:64] = np.frombuffer(np.float64(1e-7).tobytes(), dtype=np.uint8)
    h = xl.decode_header(raw)
    assert (h["S"], h["lo_sumsq"], h["level"], h["budget"], h["hi_overflow"]) == (3, 2 ** 40 + 5, 2, 1e-7, 0)


def _common(case):
    A = ex.check_exact(case)
    assert A < (1 << 51)
    xl.assert_state(case)
    R = case["R"]
    assert R["rs1"].max() < 1e10
    assert np.array_equal(case["d"], np.triu(xl.balanced_low_byte(case["X"]), 1))
    n = case["n"]
    assert np.array_equal(R["Ds"][:n, :n], case["d"] + case["d"].T)
    # e = 23 and the worst-case count from the folded W, as the library will find them
    Wu = np.ldexp(ex.fold_units(case).astype(np.float64), case["log2u"])
    assert xl.scale_exp(np.abs(np.triu(Wu, 1)).max()) == xl.E_SCALE
    assert np.abs(np.diag(Wu)).sum() == case["sumdiag"]
    return R


@pytest.mark.parametrize("n", xl.SHAPES)
@pytest.mark.parametrize("state", xl.PREP_STATES)
def test_prepare_cases_reach_their_state(n, state):
    case = xl.prep_case(n, state)
    R = _common(case)
    assert case["n_pad"] == {200: 256, 300: 512, 700: 768, 1003: 1024}[n] and R["overflow"] == 0
    assert case["decision"][3] and R["lo_sumsq"] > 0 and R["maxdiag"] > 0 and R["rs2"].max() > 0
    # the host decision from the folded matrix alone says the same
    Wu = np.ldexp(ex.fold_units(case).astype(np.float64), case["log2u"])
    S_wc, level, H, b = xl.host_decision(Wu, case["n_pad"])
    assert (S_wc, level, H, b) == (4,) + case["decision"][:3]


@pytest.mark.parametrize("n", [300, 700])
@pytest.mark.parametrize("state,plant", xl.PLANTED_CASES)
def test_planted_gram_entries_are_present(n, state, plant):
    case = xl.planted_case(n, state, plant)
    R = _common(case)
    s, half = R["shift"], 1 << (R["shift"] - 1)
    last = (n - 1) // 256 * 256
    for name, v in xl.edge_targets(s, plant).items():
        (j0, k0), (j1, k1), (j2, k2) = case["planted"][name]
        assert k0 < 256 and j1 >= last and j2 < 256 <= last <= k2       # a diagonal tile twice, an off-diagonal tile
        for j, k in case["planted"][name]:
            for a, b in ((j, k), (k, j)):                                # above and below the diagonal / the tile and its mirror
                assert R["G"][a, b] == v and R["hi"][a, b] == (v + half) >> s and R["lo"][a, b] == v - (R["hi"][a, b] << s)
    if state == "l2":
        assert R["overflow"] == 0 and (R["hi"].max(), R["hi"].min()) == (127, -128)
        assert (R["lo"] == -half).any() and (R["lo"] == half - 1).any()
    else:
        assert R["overflow"] == 1 and ((R["hi"] == 128).any(), (R["hi"] == -129).any()) == (plant != "overflow-", plant != "overflow+")
        assert (R["hi8"][R["hi"] == 128] == -128).all() and (R["hi8"][R["hi"] == -129] == 127).all()


def test_planted_maximum_is_the_row_asked_for():
    assert len(xl.LOUD_ROWS) == 27 and {0, 7, 31, 32, 127, 128, 255, 256, 287, 288, 299} <= set(xl.LOUD_ROWS)
    seen = set()
    for r in xl.LOUD_ROWS:
        case = xl.loud_case(r)
        R = _common(case)
        top = np.sort(R["rs1"])
        assert int(np.argmax(R["rs1"])) == r and top[-1] - top[-2] >= 2
        # a unit in the largest row sum moves H by more than the allowance of the round-up factors
        H_off = 0.5 * case["unit"] * (np.sqrt(float(top[-1] - 1)) + 0.5 * (case["n_pad"] - 1))
        assert H_off < case["H1"] and case["H1"] > H_off * (1 + 1e-11)
        # ... and the runner-up would give a different H still
        seen.add(case["H1"])
        assert case["decision"][:2] == (1, case["H1"])
    assert len(seen) == len(xl.LOUD_ROWS)


@pytest.mark.parametrize("name", sorted(xl.SCAN_CASES))
def test_scan_cases_miss_exactly_the_last_digit_and_stay_inside_the_bound(name):
    n, L, S_wc, state, _ = xl.SCAN_CASES[name]
    case = xl.scan_case(name)
    _common(case)
    level, H_host, b, ran2 = case["decision"]
    assert level > 0 and (S_wc < xl.SMAX - 1 or not ran2)
    # the residual of S_wc - 1 digits (round half even) is the balanced last digit, entry by entry: 2 d in units of u
    Rr = ex.digit_residual_units(case, S_wc - 1, xl.E_SCALE)
    assert np.array_equal(Rr, 2 * case["d"]) and not ex.digit_residual_units(case, S_wc, xl.E_SCALE).any()
    assert (case["d"] == -128).sum() > 10 and (case["d"] == 127).sum() > 10
    c = xl.recentre(case["Mt8"])
    miss, q2, l1 = xl.lastdigit_miss_units(case, c)
    a, vara, units = ex.scan_truth(case)
    assert np.abs(units - miss).max() < (1 << 53)
    # |miss| u <= H q2, both sides exact doubles
    err = np.ldexp(np.abs(miss).astype(np.float64), case["log2u"])
    assert np.all(err <= H_host * q2)
    assert np.count_nonzero(miss) >= L // 4
    adv = np.array(case["adv_rows"])
    assert adv.size == 6
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(q2 > 0, err / (H_host * np.maximum(q2, 1)), 0.0)
    print("%s: largest |err| / (H q2): adversarial %.4f, any marker %.4f" % (name, ratio[adv].max(), ratio.max()))
    assert 0.0 < ratio[adv].max() <= 1.0
    # zero is the commonest genotype of the adversarial and the quiet rows
    M = case["Mt8"]
    for r in list(adv) + case["quiet_rows"]:
        assert (M[r] == 0).sum() > max((M[r] == 1).sum(), (M[r] == -1).sum())
    if S_wc < 6:
        # markers on quiet individuals only: vara = W_quiet x count, and the spectral bound flags them (1 .. 64 of them), nobody sits at
        # the threshold, and the dropped digit reaches every one of them
        qr = np.array(case["quiet_rows"])
        assert qr.size == 32 and not M[np.ix_(qr, np.setdiff1d(np.arange(n), case["quiet"]))].any()
        assert np.array_equal(units[qr], (case["wq"] << -case["log2u"]) * (M[qr] != 0).sum(axis=1))
        raw = np.ldexp((units - miss).astype(np.float64), case["log2u"])
        flag, ratio_f = xl.extension_flags(raw, l1, q2, H_host, b, xl.E_SCALE, S_wc - 1)
        assert 1 <= flag[qr].sum() <= 64 and np.all(miss[flag] != 0)
        assert not np.any((ratio_f > 0.99) & (ratio_f < 1.01))
        assert flag.sum() <= 128


def test_header_expectations_by_state():
    for state, ran in (("l2", True), ("l1_default", True), ("none", True)):
        e = xl.expected_header(xl.prep_case(300, state))
        assert (e["lo_sumsq"] > 0) == ran and e["S_sliced"] == 4 and e["S"] == (4 if state == "none" else 3)
    e = xl.expected_header(xl.loud_case(0))
    assert (e["level"], e["lo_sumsq"], e["maxdiag"], e["hi_overflow"], e["S"]) == (1, 0, 0, 0, 3)
