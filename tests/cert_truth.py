"""The certificate of the digit-slice scan restated on the host (not a conftest; shared by tests/test_cert_host.py, which pins it on the
CPU, and tests/test_gpu_certificate.py).  No device work and no import of the library.

Written from the comment block above CERT_CAP in csrc/eagle_i8mfma.hip and the "Round 4" paragraphs of include/eagle_hip.h, not from the
kernels:

    b_i     the a-posteriori bound of marker i: |vara_i - m_i^T W m_i| <= b_i (bound_of below)
    LB      max_i a_i^2 / (vara_i + b_i) over the markers with finite a_i, vara_i and vara_i + b_i > 0; 0 if none is positive
    tight   how many markers with finite a_i, vara_i have b_i > 1.8 budget |vara_i| (budget: the one in force)
    a marker with finite a_i, vara_i is RE-EVALUATED in fp64 when
      (1) b_i > 1.8 B |vara_i|, B = the budget in force, or the default behind it when more than 512 markers of the WHOLE scan are over the
          tight threshold (`flagged` counts these), or
      (2) vara_i - b_i <= 0 (no upper bound of its tsq), or a_i^2 / (vara_i - b_i) >= LB (1 - 1e-9)
    at most 2,048 markers are re-evaluated; one more and the whole block is redone in fp64 (overflow).

Two behaviours the comment block leaves open, stated here as the library has them (both are on the safe side):
  * a marker whose a is NaN or Inf is skipped everywhere, also in `tight`, as one whose vara is (the fp64 kernel gives such a marker
    the same tsq, nothing to certify);
  * a term of LB that is not finite (a_i^2 overflows) is left out of the maximum.  The device drops it after its wave of 64 markers has
    been reduced, so it may lose that wave's finite terms with it: its LB is then lower, which is still a lower bound, and only this
    restatement's value is an upper limit for it (tests/test_gpu_certificate.py has the one case).

Everything is plain fp64 in the order of the comment block: (a*a)/(vara+b), (1.8*budget)*|vara|, lb*(1.0-1e-9), (a*a)/(vara-b).  These
are single IEEE operations on loaded values, the library is built without fast-math, so the block kernels return the same bits."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

CERT_CAP = 2048               # markers re-evaluated per certification; one more: the whole block in fp64
CERT_TIGHT_MAX = 512          # more markers than this over the tight threshold: the default budget is enforced
FLAG_FACTOR = 1.8             # a bound above 1.8 x budget x |vara| sends the marker to the fp64 kernel
HOEFFDING_K = 8.355           # stochastic rounding: the radius 8.355 q2 2^(e+1-8S)
SLACK = 1e-9                  # candidates are taken against LB (1 - 1e-9)
GRID_BLOCKS, BLOCK = 2048, 256
ONE_TRIP = GRID_BLOCKS * BLOCK   # 524,288 markers: the first index a thread meets on its second trip
TIGHT, LOOSE = 1e-7, 5e-7     # the budget tried first and the default behind it

Selection = namedtuple("Selection", "idx flagged overflow count")


def _f64(*xs):
    return [np.ascontiguousarray(x, dtype=np.float64) for x in xs]


def _live(a, vara):
    return np.isfinite(a) & np.isfinite(vara)


def lower_bound(a, vara, bound):
    """LB: the maximum of (a*a)/(vara+b) over the rows with finite a and vara, vara + b > 0 and a finite term; 0.0 if none is positive."""
    a, vara, bound = _f64(a, vara, bound)
    with np.errstate(all="ignore"):
        up = vara + bound
        ok = _live(a, vara) & (up > 0.0)
        t = (a[ok] * a[ok]) / up[ok]
    t = t[np.isfinite(t)]
    return float(t.max()) if t.size and t.max() > 0.0 else 0.0


def over_tight(vara, bound, budget, a=None):
    """How many finite rows have b > (1.8*budget)*|vara|.  a: rows whose a is not finite are skipped with those whose vara is not."""
    vara, bound = _f64(vara, bound)
    ok = np.isfinite(vara) if a is None else _live(_f64(a)[0], vara)
    with np.errstate(all="ignore"):
        return int((ok & (bound > (FLAG_FACTOR * float(budget)) * np.abs(vara))).sum())


def select(a, vara, bound, lb, budget, budget_loose, over_tight_all):
    """-> Selection(sorted int64 indices of the re-evaluated rows, how many of them by rule (1), count > 2,048, count).
    over_tight_all: the markers of the whole scan over the tight threshold; lb: the lower bound of the whole scan."""
    a, vara, bound = _f64(a, vara, bound)
    flag_rel = FLAG_FACTOR * float(budget_loose if over_tight_all > CERT_TIGHT_MAX else budget)
    thr = float(lb) * (1.0 - SLACK)
    with np.errstate(all="ignore"):
        ok = _live(a, vara)
        flagged = ok & (bound > flag_rel * np.abs(vara))
        den = vara - bound
        cand = ok & (~(den > 0.0) | ((a * a) / den >= thr))
    idx = np.flatnonzero(flagged | cand).astype(np.int64)
    return Selection(idx, int(flagged.sum()), int(idx.size > CERT_CAP), int(idx.size))


def select_fraction(a, v, b, slack=Fraction(1, 10 ** 9)):
    """Rule (2) alone on exact rationals (lists of Fraction, None = a row that is not finite) -> (LB, set of selected rows)."""
    rows = [i for i in range(len(a)) if a[i] is not None and v[i] is not None]
    lb = max([a[i] * a[i] / (v[i] + b[i]) for i in rows if v[i] + b[i] > 0] + [Fraction(0)])
    thr = lb * (1 - slack)
    return lb, {i for i in rows if not (v[i] - b[i] > 0) or a[i] * a[i] / (v[i] - b[i]) >= thr}


def bound_of(header, l1, q2, cshift, vdiag, mrho, vara, ext=None):
    """b_i of every marker from the decoded head of the digit workspace (exact_lastdigit.decode_header), l1_i = sum_j |m'_ij| and
    q2_i = sum_j m'_ij^2 of the re-centred marker, c_i, the diagonal term, m_i^T rho and vara_i:

        digits   round to nearest    l1^2 / 2 x delta,                      delta = 2^(e+1-8S) (0 for a diagonal W)
                 stochastic          min(8.355 q2 delta, l1^2 delta)        (never above the guaranteed bound of an interval twice as wide)
                 specH > 0           delta carries 1 + 2^-8 (the leading S digits of an (S+1)-digit rounding), and the bound is
                                     min(the above, specH q2)
                 extended marker     (ext and specH > 0: it got the dropped digit back) the rounding of S + 1 digits alone,
                                     l1^2 / 2 x delta 2^-8 / (1 + 2^-8)
        + wErr q2  (W from the int8 engine)  + 2^-48 (|diag| + |vara - diag| + [c != 0] 2 (|m^T rho| + |R|))  + 2^-50 sum_k |W_kk|."""
    l, q, c, vdiag, mrho, vara = _f64(l1, q2, cshift, vdiag, mrho, vara)
    ext = np.zeros(l.shape, dtype=bool) if ext is None else np.asarray(ext).astype(bool)
    S, e, specH, wErr = int(header["S"]), int(header["e"]), float(header["specH"]), float(header["wErr"])
    delta = float(np.ldexp(1.0, e + 1 - 8 * S)) if header["maxabs_off"] > 0.0 else 0.0
    if specH > 0.0:
        delta *= 1.0 + 2.0 ** -8
    if header["pad"]:
        b = np.minimum(HOEFFDING_K * q * delta, l * l * delta)
    else:
        b = 0.5 * l * l * delta
    if specH > 0.0:
        b = np.minimum(b, specH * q)
        b = np.where(ext, 0.5 * l * l * (delta * (2.0 ** -8 / (1.0 + 2.0 ** -8))), b)
    mag = np.abs(vdiag) + np.abs(vara - vdiag)
    mag = np.where(c != 0, mag + 2.0 * (np.abs(mrho) + abs(float(header["R"]))), mag)
    return b + wErr * q + 2.0 ** -48 * mag + 2.0 ** -50 * float(header["sumdiag"])


def bound_of_loops(header, l1, q2, cshift, vdiag, mrho, vara, ext=None):
    """bound_of, one marker at a time in Python floats (tests/test_cert_host.py holds the two against each other)."""
    out = []
    for i in range(len(l1)):
        l, q = float(l1[i]), float(q2[i])
        delta = 2.0 ** (header["e"] + 1 - 8 * header["S"]) if header["maxabs_off"] > 0 else 0.0
        if header["specH"] > 0:
            delta = delta * (1.0 + 1.0 / 256.0)
        if ext is not None and ext[i] and header["specH"] > 0:
            b = 0.5 * l * l * (delta * ((1.0 / 256.0) / (1.0 + 1.0 / 256.0)))
        else:
            b = min(HOEFFDING_K * q * delta, l * l * delta) if header["pad"] else 0.5 * l * l * delta
            if header["specH"] > 0:
                b = min(b, header["specH"] * q)
        mag = abs(float(vdiag[i])) + abs(float(vara[i]) - float(vdiag[i]))
        if cshift[i] != 0:
            mag += 2.0 * (abs(float(mrho[i])) + abs(header["R"]))
        out.append(b + header["wErr"] * q + 2.0 ** -48 * mag + 2.0 ** -50 * header["sumdiag"])
    return np.array(out, dtype=np.float64)


def fabricated_header(budget=TIGHT, budget_loose=LOOSE):
    """256 zero bytes with the two doubles the block kernels read from the head of the digit workspace (exact_lastdigit.HEADER_FIELDS:
    budget at 56, budget_loose at 112)."""
    raw = np.zeros(256, dtype=np.uint8)
    raw[56:64] = np.frombuffer(np.float64(budget).tobytes(), dtype=np.uint8)
    raw[112:120] = np.frombuffer(np.float64(budget_loose).tobytes(), dtype=np.uint8)
    return raw


# ---- planted arrays ---------------------------------------------------------------------------------------------------------------------
UP, DOWN = np.inf, -np.inf
PEAK = 256.0                                   # a^2 / vara of the planted maximum; the base rows stay below 64 / (1 - 1e-9)


def thr_of(lb):
    return float(lb) * (1.0 - SLACK)


def lb_with_threshold(q):
    """A double lb with lb*(1.0-1e-9) == q exactly.  (1 - 1e-9 < 1: the products of neighbouring doubles are less than one unit in the last
    place apart, so no double is stepped over.)"""
    lb = np.float64(q) / (1.0 - SLACK)
    for _ in range(64):
        p = lb * (1.0 - SLACK)
        if p == q:
            return float(lb)
        lb = np.nextafter(lb, UP if p < q else DOWN)
    raise AssertionError("no lb whose threshold is %r" % q)


def row_with_quotient(a, b, target):
    """A double vara with (a*a)/(vara-b) == target exactly: the quotient falls by less than one unit in the last place of target per
    step of vara wherever ulp(vara) / vara < ulp(target) / target (asserted), so none is stepped over."""
    a, b, target = np.float64(a), np.float64(b), np.float64(target)
    v = (a * a) / target + b
    assert np.spacing(v) / v < np.spacing(target) / target
    for _ in range(16):
        v = np.nextafter(v, DOWN)
    for _ in range(64):
        qt = (a * a) / (v - b)
        if qt == target:
            return float(v)
        assert qt > target, "started above the target and never met it"
        v = np.nextafter(v, UP)
    raise AssertionError("no vara with quotient %r" % target)


EDGE_Q = 300.0078125 * 1.0000001               # the knife-edge value of a^2 / (vara - b): above PEAK, nothing special about its bits
KINDS = ("peak", "a_nan", "a_pinf", "a_ninf", "v_nan", "v_pinf", "v_ninf", "up_zero", "den_zero", "den_neg", "v_neg", "a_zero", "b_zero_tie",
         "b_zero_below", "flag_at", "flag_above", "cand_at", "cand_below")


def _kind_row(kind, budget):
    """(a, vara, b) of one planted row.  Rows that must be SKIPPED carry what would select them if they were not: a huge bound (a_nan:
    flagged), an infinite or NaN quotient (the others)."""
    flag = FLAG_FACTOR * budget
    if kind == "peak":                         # the maximum: a^2 / (v + b) just under 256
        return 16.0, 1.0, 2.0 ** -40
    if kind == "a_nan":
        return np.nan, 1.0, 1e-3
    if kind == "a_pinf":
        return np.inf, 1.0, 1e-9
    if kind == "a_ninf":
        return -np.inf, 1.0, 1e-9
    if kind == "v_nan":
        return 1000.0, np.nan, 1e-9
    if kind == "v_pinf":
        return 1000.0, np.inf, 1e-9
    if kind == "v_ninf":
        return 1000.0, -np.inf, 1e-9
    if kind == "up_zero":                      # vara + b = 0: no term of LB; vara - b < 0: re-evaluated
        return 3.0, -1.0, 1.0
    if kind == "den_zero":                     # vara - b = 0
        return 3.0, 1.0, 1.0
    if kind == "den_neg":                      # vara - b < 0 < vara
        return 3.0, 1.0, 1.5
    if kind == "v_neg":                        # vara < 0 with a small bound: no term of LB, re-evaluated
        return 3.0, -2.0, 2.0 ** -30
    if kind == "a_zero":                       # a candidate only against lb = 0
        return 0.0, 1.0, 2.0 ** -30
    if kind == "b_zero_tie":                   # b = 0 and a^2 / vara = 256: sets LB and is its own candidate
        return -16.0, 1.0, 0.0
    if kind == "b_zero_below":                 # b = 0, 1e-8 below the threshold
        return 16.0, 1.0 + 1e-8, 0.0
    if kind == "flag_at":                      # b == 1.8 budget |vara| to the bit: NOT flagged
        return 1.0, 3.7, flag * 3.7
    if kind == "flag_above":                   # one unit in the last place above: flagged
        return 1.0, 3.7, float(np.nextafter(np.float64(flag * 3.7), UP))
    b = 2.0 ** -30
    if kind == "cand_at":                      # (a*a)/(vara-b) == EDGE_Q to the bit: a candidate when the threshold is EDGE_Q
        return 17.25, row_with_quotient(17.25, b, np.float64(EDGE_Q)), b
    if kind == "cand_below":                   # one unit in the last place below: not one
        return 17.25, row_with_quotient(17.25, b, np.nextafter(np.float64(EDGE_Q), DOWN)), b
    raise KeyError(kind)


def anchors(L):
    """Where planted rows go: from index 0 up, from L - 1 down, and on both sides of the 524,288th marker (the second grid trip)."""
    out = [("head", 0, 1)]
    if L > ONE_TRIP:
        out += [("below_trip", ONE_TRIP - 1, -1), ("from_trip", ONE_TRIP, 1)]
    return out + [("tail", L - 1, -1)]


def base_arrays(L, seed):
    """Seeded rows none of which is selected against a lower bound of 256 or more under the tight budget: a^2 / (vara - b) < 64.001 and
    b <= 1e-9 vara."""
    rng = np.random.default_rng(1000003 * seed + L)
    vara = rng.uniform(1.0, 2.0, L)
    bound = vara * rng.uniform(1e-10, 1e-9, L)
    a = rng.uniform(-8.0, 8.0, L)
    return a, vara, bound


def edge_case(L, seed=1, budget=TIGHT, budget_loose=LOOSE):
    """Every kind of KINDS at every anchor that has room for it (a short array gets the first kinds only) -> dict(a, vara, bound, budget,
    budget_loose, rows {(anchor, kind): index})."""
    a, vara, bound = base_arrays(L, seed)
    rows, taken = {}, set()
    for name, start, step in anchors(L):
        i = start
        for kind in KINDS:
            while i in taken:
                i += step
            if not 0 <= i < L:
                break
            a[i], vara[i], bound[i] = _kind_row(kind, budget)
            rows[(name, kind)] = i
            taken.add(i)
            i += step
    return dict(a=a, vara=vara, bound=bound, budget=budget, budget_loose=budget_loose, rows=rows)


def spread(L, k, seed):
    """k distinct rows of [0, L): both ends, both sides of the second grid trip, the rest seeded."""
    assert 0 <= k <= L
    fixed = [i for i in (0, L - 1, ONE_TRIP - 1, ONE_TRIP, 255, 256) if 0 <= i < L]
    fixed = list(dict.fromkeys(fixed))[:k]
    rng = np.random.default_rng(7919 * seed + L + k)
    rest = np.setdiff1d(np.arange(L), np.array(fixed, dtype=np.int64))
    more = rng.choice(rest, size=k - len(fixed), replace=False) if k > len(fixed) else np.array([], dtype=np.int64)
    return np.sort(np.concatenate([np.array(fixed, dtype=np.int64), more]))


def cap_case(L, k, seed=2, budget=TIGHT, budget_loose=LOOSE):
    """Exactly k qualifying rows (all tied at the maximum, a = +-16, vara = 1, b = 2^-40) spread over the array."""
    a, vara, bound = base_arrays(L, seed)
    at = spread(L, k, seed)
    a[at] = np.where(at % 2 == 0, 16.0, -16.0)
    vara[at], bound[at] = 1.0, 2.0 ** -40
    return dict(a=a, vara=vara, bound=bound, budget=budget, budget_loose=budget_loose, rows={("spread", "tie"): at})


def tier_case(L, m, seed=3, budget=TIGHT, budget_loose=LOOSE, rel=3e-7):
    """One peak and m rows with b = 3e-7 |vara|: over the tight threshold 1.8e-7, under the default one 9e-7, nowhere near the maximum."""
    a, vara, bound = base_arrays(L, seed)
    at = spread(L, m + 1, seed)
    peak, at = at[len(at) // 2], np.delete(at, len(at) // 2)
    a[peak], vara[peak], bound[peak] = 16.0, 1.0, 2.0 ** -40
    bound[at] = rel * vara[at]
    return dict(a=a, vara=vara, bound=bound, budget=budget, budget_loose=budget_loose, rows={("spread", "between"): at, ("spread", "peak"): peak})


def inf_case(L=1000, seed=4, budget=TIGHT, budget_loose=LOOSE):
    """a^2 overflows for one marker (row 70) whose wave of 64 also holds the finite maximum (row 100); a smaller peak sits in another
    wave (row 300)."""
    a, vara, bound = base_arrays(L, seed)
    a[70], vara[70], bound[70] = 1e200, 1.0, 2.0 ** -30
    a[100], vara[100], bound[100] = 16.0, 1.0, 2.0 ** -40
    a[300], vara[300], bound[300] = 12.0, 1.0, 2.0 ** -40
    return dict(a=a, vara=vara, bound=bound, budget=budget, budget_loose=budget_loose, rows={("w1", "overflow"): 70, ("w1", "peak"): 100, ("w4", "peak"): 300})


def predict(case, lb=None, over_tight_all=None):
    """What the block flow must return for a planted case: dict(lower_bound, over_tight, sel) -- lb / over_tight_all as handed to the
    selection (None: the block's own)."""
    own = lower_bound(case["a"], case["vara"], case["bound"])
    tight = over_tight(case["vara"], case["bound"], case["budget"], case["a"])
    sel = select(case["a"], case["vara"], case["bound"], own if lb is None else lb, case["budget"], case["budget_loose"],
                 tight if over_tight_all is None else over_tight_all)
    return dict(lower_bound=own, over_tight=tight, sel=sel)
