"""CPU: the certificate's rule as tests/cert_truth.py restates it -- its constants against the source text of csrc/eagle_i8mfma.hip, its
soundness on exact rationals, its bound against plain loops, and its planted arrays against what they are built to hold -- so that
tests/test_gpu_certificate.py compares the device with a truth that is right.  No device work."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import cert_truth as ct
import exact_lastdigit as xl
from conftest import ROOT


def source(name="eagle_i8mfma.hip"):
    return open(os.path.join(ROOT, "eagleeverything_amd", "csrc", name)).read()


def test_constants_are_the_source_text():
    s = source()
    defines = s
    s = s[s.index("// Certification of a digit-slice scan"):s.index("__global__ void k_vara_i8_bound(")]     # the certificate's layer
    assert int(re.search(r"#define\s+CERT_CAP\s+(\d+)\s", s).group(1)) == ct.CERT_CAP
    assert int(re.search(r"#define\s+CERT_TIGHT_MAX\s+(\d+)\s", s).group(1)) == ct.CERT_TIGHT_MAX
    assert float(re.search(r"#define\s+VARA_FLAG_FACTOR\s+([0-9.]+)\s", defines).group(1)) == ct.FLAG_FACTOR == xl.FLAG_FACTOR
    assert float(re.search(r"#define\s+VARA_HOEFFDING_K\s+([0-9.]+)\s", defines).group(1)) == ct.HOEFFDING_K
    # the slack, the two caps and the tier rule, in both flows
    slack = re.findall(r"const double thr = lb \* \(1\.0 - ([0-9.e+-]+)\);", s)
    assert len(slack) == 2 and all(float(x) == ct.SLACK for x in slack)
    assert s.count("const bool cand = !(den > 0.0) || (x * x) / den >= thr;") == 2
    assert s.count("if (k < CERT_CAP) idx[k] = i; else ch->overflow = 1;") == 2
    assert "ch->tight > CERT_TIGHT_MAX ? cc.flag_loose : cc.flag_rel" in s and "over_tight > CERT_TIGHT_MAX ? 1 : 0" in s
    assert s.count("if (!(isfinite(x) && isfinite(v))) continue;") == 4 and s.count("if (!(up > 0.0)) continue;") == 2
    # the grid of all five kernels: 2,048 blocks of 256 at the most, each thread striding by the grid
    assert s.count("if (blocks > %d) blocks = %d;" % (ct.GRID_BLOCKS, ct.GRID_BLOCKS)) == 5
    assert s.count("unsigned blocks = (unsigned)((L + 255) / 256);") == 5
    assert s.count("i < L; i += (long)gridDim.x * %d" % ct.BLOCK) == 5 and ct.ONE_TRIP == 524288
    for k in ("k_cert_lb", "k_cert_select", "k_cert_bounds", "k_cert_lb_b", "k_cert_select_b"):
        assert re.search(r"hipLaunchKernelGGL\(%s, dim3\(blocks\), dim3\(256\)" % k, s), k
    # the index list behind a 256-byte head, the budgets the block kernels read from the head of the digit workspace
    assert "static size_t cert_idx_off() { return 256; }" in s and "hipMemsetAsync(cert_ws, 0, 256, s)" in s
    fields = {name: (off, kind) for name, off, kind in xl.HEADER_FIELDS}
    assert fields["budget"] == (56, "f8") and fields["budget_loose"] == (112, "f8")
    raw = ct.fabricated_header(1e-7, 5e-7)
    hdr = xl.decode_header(raw)
    assert hdr["budget"] == 1e-7 and hdr["budget_loose"] == 5e-7 and not raw[:56].any() and not raw[64:112].any() and not raw[120:].any()
    assert (ct.TIGHT, ct.LOOSE) == (xl.TIGHT, xl.BUDGET)


# ---- soundness on exact rationals ----------------------------------------------------------------------------------------------------
E9, E10 = Fraction(1, 10 ** 9), Fraction(1, 10 ** 10)


def _draw(rng, N=9):
    """One panel: (a, t, b, v), lists of Fraction with None for a row that is not finite.  Contenders sit within a few 1e-9 of each other
    with bounds of that size; exact ties, rows with v - b <= 0, rows with b = 0 and rows far below are mixed in."""
    a, t, b, v = [], [], [], []
    for i in range(N):
        kind = rng.choice(["contender", "contender", "contender", "tie", "low", "wide", "exact", "skipped"]) if i else "contender"
        if kind == "tie" and any(x is not None for x in a):
            j = int(rng.choice([k for k in range(i) if a[k] is not None]))
            a.append(a[j] * int(rng.choice([-1, 1]))), t.append(t[j]), b.append(b[j]), v.append(v[j])
            continue
        if kind == "skipped":
            a.append(None), t.append(None), b.append(None), v.append(None)
            continue
        ai = Fraction(int(rng.choice([-3, 3])))
        ti = 2 * (1 + int(rng.integers(-6, 7)) * E9)
        bi = ti * int(rng.choice([0, 1, 2, 5, 40])) * E9
        if kind == "low":
            ai = Fraction(int(rng.choice([-2, -1, 0, 1, 2])))
        if kind == "wide":                                   # the bound swallows the value
            bi = ti * int(rng.choice([1, 2, 3]))
        if kind == "exact":
            bi = Fraction(0)
        vi = ti + bi * Fraction(int(rng.integers(-4, 5)), 4)  # |v - t| <= b, the ends included
        a.append(ai), t.append(ti), b.append(bi), v.append(vi)
    return a, t, b, v


def _first_argmax(a, x):
    best, at = None, -1
    for i in range(len(a)):
        if a[i] is None or x[i] is None or x[i] == 0:
            continue
        q = a[i] * a[i] / x[i]
        if best is None or q > best:
            best, at = q, i
    return at, best


def _property(a, t, b, v, eps):
    """-> (holds, selected): the certified array [fp64 value of the selected, digit value of the others] has the first arg-max of the
    array in which everybody carries the fp64 value, and every unselected marker is strictly below the winner in both."""
    lb, sel = ct.select_fraction(a, v, b)
    f64 = [None if t[i] is None else t[i] * (1 + eps[i]) for i in range(len(a))]
    cert = [f64[i] if i in sel else v[i] for i in range(len(a))]
    w_c, top_c = _first_argmax(a, cert)
    w_f, top_f = _first_argmax(a, f64)
    ok = w_c == w_f and w_c in sel
    for i in range(len(a)):
        if a[i] is None or i in sel:
            continue
        ok = ok and a[i] * a[i] / cert[i] < top_c and a[i] * a[i] / f64[i] < top_f
    return ok, sel


def test_selection_is_sound_on_exact_rationals():
    """With t_i the true quadratic form (t_i > 0), |v_i - t_i| <= b_i and the fp64 kernel returning t_i (1 + eps_i), |eps_i| <= e:

        LB = max_j a_j^2 / (v_j + b_j) <= T = max_j a_j^2 / t_j                     (t_j <= v_j + b_j)
        the marker that attains T is selected: a^2 / (v - b) >= a^2 / t = T >= LB >= LB (1 - s), or v - b <= 0
        an UNSELECTED marker i has v_i - b_i > 0 and a_i^2 / (v_i - b_i) < LB (1 - s), so both its digit value a_i^2 / v_i and its true
        value a_i^2 / t_i are below T (1 - s); its fp64 value is below T (1 - s) / (1 - e)
        the winner of the fp64 array is at least T / (1 + e)

    so unselected markers are strictly below the winner of either array as soon as (1 - s) / (1 - e) <= 1 / (1 + e), i.e.
    2 e <= s (1 + e): the slack s = 1e-9 pays for 2 |eps| < 1e-9, and the fp64 kernel's own rounding (a few hundred roundings of 1.1e-16)
    is far inside 4e-10.  Both arrays then have their maximum among the selected markers, which carry the same values in both: the same
    first arg-max.  At |eps| = 1e-9 the property fails (the last case below): the slack is what buys it."""
    rng = np.random.default_rng(20240917)
    seen = dict(unselected=0, ties=0, wide=0, exact=0, skipped=0, near=0)
    for trial in range(3000):
        a, t, b, v = _draw(rng)
        eps = [None if x is None else int(rng.integers(-4, 5)) * E10 for x in a]
        ok, sel = _property(a, t, b, v, eps)
        assert ok, (trial, a, t, b, v, eps)
        live = [i for i in range(len(a)) if a[i] is not None]
        assert not (set(range(len(a))) - set(live)) & sel
        seen["unselected"] += len(live) - len(sel)
        seen["skipped"] += len(a) - len(live)
        seen["wide"] += sum(1 for i in live if v[i] - b[i] <= 0)
        seen["exact"] += sum(1 for i in live if b[i] == 0)
        seen["ties"] += sum(1 for i in live for j in live if i < j and a[i] ** 2 * v[j] == a[j] ** 2 * v[i])
        seen["near"] += max(0, sum(1 for i in sel if v[i] - b[i] > 0) - 1)     # near-ties inside b, beside the winner
        assert all(v[i] - b[i] > 0 or i in sel for i in live)
    assert min(seen.values()) > 300, seen
    # what the slack buys: marker 1 sits just under LB (1 - 1e-9) and is left alone; with fp64 values 1e-9 off it wins the fp64 array
    d = Fraction(1, 10 ** 12)
    a = [Fraction(1), Fraction(1)]
    t = [Fraction(1), 1 / ((1 - E9) * (1 - d))]
    b = [Fraction(0), Fraction(0)]
    lb, sel = ct.select_fraction(a, t, b)
    assert lb == 1 and sel == {0}
    assert _property(a, t, b, t, [4 * E10, -4 * E10])[0]
    assert not _property(a, t, b, t, [E9, -E9])[0]


def test_fp64_rule_is_the_rational_rule_away_from_the_edges():
    """select / lower_bound in fp64 against select_fraction on the same doubles taken as exact rationals (dyadic: Fraction(x) is exact):
    the sets agree wherever no quotient lies within 1e-12 of the threshold, and the lower bound to 4 units in the last place."""
    rng = np.random.default_rng(5)
    for trial in range(300):
        N = 12
        v = rng.uniform(1.0, 2.0, N)
        b = v * rng.choice([0.0, 1e-9, 3e-9, 0.6, 1.0, 1.5], size=N)
        a = rng.choice([3.0, -3.0, 1.0, 0.0], size=N) * (1 + rng.integers(-3, 4, N) * 1e-9)
        a[rng.integers(N)] = np.nan
        v[rng.integers(N)] = np.inf
        fa = [None if not np.isfinite(x) else Fraction(float(x)) for x in a]
        fv = [None if not np.isfinite(x) else Fraction(float(x)) for x in v]
        fb = [Fraction(float(x)) for x in b]
        lb_q, sel_q = ct.select_fraction(fa, fv, fb)
        lb = ct.lower_bound(a, v, b)
        assert abs(Fraction(lb) - lb_q) <= lb_q * Fraction(4, 2 ** 52)
        sel = ct.select(a, v, b, lb, 1.0, 1.0, 0)              # budget 1: nobody is flagged
        assert sel.flagged == 0 and sel.overflow == 0 and sel.count == sel.idx.size
        thr = lb_q * (1 - E9)
        edge = {i for i in range(N) if fa[i] is not None and fv[i] is not None and fv[i] - fb[i] > 0
                and abs(fa[i] ** 2 / (fv[i] - fb[i]) - thr) <= thr * Fraction(1, 10 ** 12)}
        assert set(sel.idx.tolist()) - edge == sel_q - edge, (trial, sel.idx, sel_q, edge)


# ---- the bound ------------------------------------------------------------------------------------------------------------------------
def _hdr(**kw):
    h = dict(maxabs_off=0.75, S=3, pad=0, bound=0.0, sumdiag=800.0, R=-12.5, specH=0.0, S_sliced=3, budget=1e-7, e=0, wErr=0.0,
             budget_loose=5e-7)
    h.update(kw)
    return h


SPECH = 1e-6
BRANCHES = {"nearest": _hdr(), "stochastic": _hdr(pad=1, S=2, S_sliced=2), "spectral": _hdr(specH=SPECH, S=3, S_sliced=4),
            "extended": _hdr(specH=SPECH, S=3, S_sliced=4), "w8": _hdr(wErr=2e-12), "diagonal": _hdr(maxabs_off=0.0)}


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_bound_of_against_plain_loops(branch):
    h = BRANCHES[branch]
    rng = np.random.default_rng(len(branch))
    N = 40
    q2 = rng.integers(1, 400, N)
    l1 = q2 + rng.integers(0, 50, N)                         # (any pair will do here; real markers have l1 <= q2 <= 2 l1)
    l1[:4], q2[:4] = [1, 2, 300, 20], [1, 4, 300, 40]         # small rows: the stochastic minimum and the spectral minimum switch sides
    c = rng.integers(-1, 2, N)
    vdiag, mrho = rng.uniform(50, 90, N), rng.uniform(-30, 30, N)
    vara = vdiag + rng.uniform(-40, 5, N)
    ext = (np.arange(N) % 3 == 0) if branch == "extended" else None
    got = ct.bound_of(h, l1, q2, c, vdiag, mrho, vara, ext)
    want = ct.bound_of_loops(h, l1, q2, c, vdiag, mrho, vara, ext)
    assert np.array_equal(got, want)
    # by hand, marker 3 (l1 = 20, q2 = 40)
    delta = {"nearest": 2.0 ** -23, "stochastic": 2.0 ** -15, "spectral": 2.0 ** -23 * (1 + 2.0 ** -8), "extended": 2.0 ** -31, "w8": 2.0 ** -23,
             "diagonal": 0.0}[branch]
    lead = {"nearest": 200 * delta, "stochastic": min(8.355 * 40 * delta, 400 * delta), "spectral": min(200 * delta, SPECH * 40),
            "extended": 200 * delta, "w8": 200 * delta + 2e-12 * 40, "diagonal": 0.0}[branch]
    mag = abs(vdiag[3]) + abs(vara[3] - vdiag[3]) + (2 * (abs(mrho[3]) + 12.5) if c[3] else 0.0)
    assert got[3] == pytest.approx(lead + 2.0 ** -48 * mag + 2.0 ** -50 * 800.0, rel=1e-14)
    if branch == "stochastic":                                # both sides of the minimum are met
        assert 8.355 * q2[0] * delta > l1[0] ** 2 * delta and 8.355 * q2[2] * delta < l1[2] ** 2 * delta
    if branch == "spectral":
        assert 0.5 * l1[0] ** 2 * delta < SPECH * q2[0] and 0.5 * l1[2] ** 2 * delta > SPECH * q2[2]
    if branch == "extended":                                  # the others keep the spectral branch
        assert np.array_equal(got[~ext], ct.bound_of(h, l1, q2, c, vdiag, mrho, vara)[~ext]) and (got[ext] != ct.bound_of(h, l1, q2, c, vdiag, mrho, vara)[ext]).all()
        assert np.array_equal(ct.bound_of(_hdr(), l1, q2, c, vdiag, mrho, vara, ext), ct.bound_of(_hdr(), l1, q2, c, vdiag, mrho, vara))


# ---- the planted arrays -----------------------------------------------------------------------------------------------------------------
def test_knife_edge_helpers():
    q = np.float64(ct.EDGE_Q)
    lb = ct.lb_with_threshold(q)
    assert lb * (1.0 - 1e-9) == q and ct.thr_of(lb) == q and lb > ct.PEAK
    for target in (q, np.nextafter(q, -np.inf)):
        v = ct.row_with_quotient(17.25, 2.0 ** -30, target)
        assert (17.25 * 17.25) / (np.float64(v) - 2.0 ** -30) == target
    flag = ct.FLAG_FACTOR * ct.TIGHT
    a, v, b = ct._kind_row("flag_at", ct.TIGHT)
    assert b == flag * abs(v) and not b > flag * abs(v)
    a, v, b2 = ct._kind_row("flag_above", ct.TIGHT)
    assert b2 > flag * abs(v) and b2 == np.nextafter(b, np.inf)


@pytest.mark.parametrize("L", [0, 1, 255, 256, 257, 524288, 524289, 1000003])
def test_edge_case_holds_what_it_is_built_to_hold(L):
    case = ct.edge_case(L)
    rows = case["rows"]
    names = {n for n, _ in rows}
    assert names == ({"head", "tail", "below_trip", "from_trip"} if L > ct.ONE_TRIP else {"head", "tail"} if L > 1 else {"head"} if L else set())
    if L >= 2 * len(ct.KINDS):
        short = max(0, len(ct.KINDS) - (L - ct.ONE_TRIP)) if L > ct.ONE_TRIP else 0          # 524,289: one row from the second trip on
        assert len(rows) == len(ct.KINDS) * len(names) - short == len(set(rows.values()))
        assert rows[("head", "peak")] == 0 and L - 1 in (rows[("tail", "peak")], rows.get(("from_trip", "peak")))
    if L > ct.ONE_TRIP + len(ct.KINDS):
        assert rows[("below_trip", "peak")] == ct.ONE_TRIP - 1 and rows[("from_trip", "peak")] == ct.ONE_TRIP
    planted = np.array(sorted(rows.values()), dtype=np.int64)
    kind_at = {i: k for (_, k), i in rows.items()}
    a, vara, bound = case["a"], case["vara"], case["bound"]
    # against the block's own lower bound: the b = 0 tie sets it (256), the knife-edge rows (300) are above it
    p = ct.predict(case)
    has = lambda k: any(kk == k for _, kk in rows)
    want_lb = (17.25 * 17.25) / (vara[rows[("head", "cand_at")]] + 2.0 ** -30) if has("cand_at") else 256.0 if has("b_zero_tie") else \
        256.0 / (1.0 + 2.0 ** -40) if L else 0.0
    assert p["lower_bound"] == pytest.approx(want_lb, rel=1e-15)
    assert set(p["sel"].idx.tolist()) <= set(planted.tolist())          # no candidate beyond the planted ones
    skipped = {"a_nan", "a_pinf", "a_ninf", "v_nan", "v_pinf", "v_ninf"}
    assert not {kind_at[i] for i in p["sel"].idx.tolist()} & skipped
    always = {"up_zero", "den_zero", "den_neg", "v_neg", "flag_above"}
    assert {k for k in always if has(k)} <= {kind_at[i] for i in p["sel"].idx.tolist()}
    n_of = lambda k: sum(1 for _, kk in rows if kk == k)
    assert p["over_tight"] == sum(n_of(k) for k in ("up_zero", "den_zero", "den_neg", "flag_above")) == p["sel"].flagged
    # the threshold on the knife edge: cand_at is in, cand_below is out, the peaks (256) are out, flag_at never is in
    if has("cand_below"):
        p = ct.predict(case, lb=ct.lb_with_threshold(np.float64(ct.EDGE_Q)))
        kinds = [kind_at[i] for i in p["sel"].idx.tolist()]
        assert kinds.count("cand_at") == n_of("cand_at") and "cand_below" not in kinds and "peak" not in kinds and "flag_at" not in kinds
        assert set(kinds) == always | {"cand_at"}
    # lb = 0: every finite row, a = 0 included
    p = ct.predict(case, lb=0.0)
    finite = int((np.isfinite(a) & np.isfinite(vara)).sum())
    assert p["sel"].count == finite == L - sum(n_of(k) for k in skipped) and p["sel"].overflow == int(finite > 2048)


def test_cap_tier_and_overflow_cases_hold_their_counts():
    for L in (524288, 1000003):
        for k in (2048, 2049):
            case = ct.cap_case(L, k)
            p = ct.predict(case)
            at = case["rows"][("spread", "tie")]
            assert p["sel"].count == k and p["sel"].overflow == int(k > 2048) and np.array_equal(p["sel"].idx, at) and p["sel"].flagged == 0
            assert {0, L - 1} <= set(at.tolist()) and (L <= ct.ONE_TRIP or {ct.ONE_TRIP - 1, ct.ONE_TRIP} <= set(at.tolist()))
            assert p["lower_bound"] == 256.0 / (1.0 + 2.0 ** -40) and p["over_tight"] == 0
    for L, m in ((257, 100), (1000003, 700)):
        case = ct.tier_case(L, m)
        between, peak = case["rows"][("spread", "between")], case["rows"][("spread", "peak")]
        assert ct.predict(case)["over_tight"] == m == between.size
        p = ct.predict(case, over_tight_all=512)
        assert p["sel"].flagged == m and p["sel"].count == m + 1 and set(p["sel"].idx.tolist()) == set(between.tolist()) | {int(peak)}
        p = ct.predict(case, over_tight_all=513)
        assert p["sel"].flagged == 0 and p["sel"].idx.tolist() == [int(peak)]
    case = ct.inf_case()
    p = ct.predict(case)
    assert p["lower_bound"] == 256.0 / (1.0 + 2.0 ** -40) and p["sel"].idx.tolist() == [70, 100]
    assert 70 // 64 == 100 // 64 != 300 // 64
