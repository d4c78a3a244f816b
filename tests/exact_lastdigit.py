"""Operands whose LAST digit is chosen, and the spectral bound of that digit restated in integers
(not a conftest; shared by tests/test_lastdigit_exact_host.py, which pins it on the CPU, tests/test_gpu_lastdigit_exact.py,
tests/test_gpu_spectral.py and tests/test_gpu_gram_once.py).

The operands are those of tests/exact_scan.py (S = I, V = u X with X a symmetric int64 matrix, a_hat integer: every a and vara an integer
times a power of two that fp64 holds), with three more handles:

    diag_scale / state   the integer diagonal is max(dominance value, a chosen magnitude): sum_k |W_kk| steers the worst-case digit count
                         S_wc and which level of the spectral bound passes (k_vara_prep and k_spectral_decide read only sumdiag, n_pad, e and
                         the row sums), so a case can be put into any state of the digit rule; `state` solves the magnitude from the
                         restatement below
    the last digit       u = 2^(24 - 8 S_wc) and e = 23: the unit of digit S_wc of the folded entries 2 W_jk is 2 u, so the last digit of the
                         pair (j, k) is the balanced low byte of X_jk.  X_jk = 256 h_jk + d_jk with d placed and h random (even where
                         d = -128, so that round-half-even on S_wc - 1 digits agrees with the balanced digit's carry)
    quiet                individuals without off-diagonal entries and with a small integer diagonal: a marker that is non-zero only on
                         them has vara = W_quiet * (its non-zero count), far below q2 x a typical W_kk, and fails its budget under
                         the spectral bound.  (k_marker_shift centres such a marker on its commoner homozygote, c = +-1, so its
                         re-centred row covers everybody and the dropped digit does reach it.)

and the host restatement of what csrc/eagle_i8mfma.hip leaves behind on the automatic path -- k_slice_w's symmetric image Ds, the Gram
product G = Ds Ds, its row sums, E_hi / lo_sumsq / maxdiag / hi_overflow of the fused epilogue, the row sums of |E_hi E_hi|, H1 and H2 and
the order of decisions of k_spectral_decide -- all of it integer arithmetic up to the two square roots of the bound itself."""
import numpy as np

import exact_scan as ex

SMAX = 7                       # slots of the slice area with an automatic digit count
BUDGET, TIGHT = 5e-7, 1e-7     # the library's default budget and the tight one it tries first
FLAG_FACTOR = 1.8              # what the certificate and the extension enforce per marker: a bound above 1.8 x budget x |vara|
LOG2U_OF_SLICES = {4: -8, 5: -16, 6: -24}   # u = 2^(24 - 8 S_wc)
E_SCALE = 23                   # the scale exponent the planted 2^22 - 1 fixes

HEADER_FIELDS = (("maxabs_off", 0, "f8"), ("S", 8, "i4"), ("pad", 12, "i4"), ("bound", 16, "f8"), ("sumdiag", 24, "f8"), ("R", 32, "f8"),
                 ("specH", 40, "f8"), ("S_sliced", 48, "i4"), ("budget", 56, "f8"), ("e", 64, "i4"), ("lo_sumsq", 72, "u8"), ("maxdiag", 80, "i4"),
                 ("hi_overflow", 84, "i4"), ("spec_try2", 88, "i4"), ("level", 92, "i4"), ("wErr", 96, "f8"), ("specH1", 104, "f8"),
                 ("budget_loose", 112, "f8"))


def decode_header(raw):
    """The head of the digit workspace (VaraHdr, csrc/eagle_internal.h: 120 bytes) as a dict of Python numbers."""
    h = np.asarray(raw[:120], dtype=np.uint8).tobytes()
    out = {}
    for name, off, kind in HEADER_FIELDS:
        x = np.frombuffer(h[off:off + int(kind[1])], dtype=np.dtype("<" + kind))[0]
        out[name] = float(x) if kind == "f8" else int(x)
    return out


def pad256(n):
    return (n + 255) // 256 * 256


def gram_shift(n_pad):
    """s of E_hi = round(offdiag(Ds Ds) / 2^s) (vara_i8_prepare_impl): 127 x 2^s holds 8 standard deviations of a random Gram entry."""
    shift = 8
    while shift < 23 and 127.0 * (1 << shift) < 8.0 * 5476.0 * np.sqrt(n_pad):
        shift += 1
    return shift


def balanced_low_byte(X):
    return ((X + 128) & 255) - 128


def _int_gram(A):
    """A A for a symmetric integer matrix with |entries| <= 128 and at most 2^10 rows: one fp64 product, exact (|sums| < 2^25)."""
    Af = A.astype(np.float64)
    G = Af @ Af
    assert np.abs(G).max(initial=0) < 2.0 ** 52
    return G.astype(np.int64)


def restate(d, n_pad):
    """d: the last digits above the diagonal (N x N int64, N <= n_pad, zero on and below the diagonal) -> everything the prepare step
    derives from them, in integers: Ds (n_pad x n_pad), G, rs1, shift, E, hi, lo, lo_sumsq, maxdiag, overflow, hi8 (the int8 image the
    device stores: wrapped where hi left int8), rs2 (row sums of |hi8 hi8|)."""
    N = d.shape[0]
    assert N <= n_pad and not np.tril(d).any() and np.abs(d).max(initial=0) <= 128
    Ds = np.zeros((n_pad, n_pad), dtype=np.int64)
    Ds[:N, :N] = d + d.T
    G = _int_gram(Ds)
    rs1 = np.abs(G).sum(axis=1)
    shift = gram_shift(n_pad)
    half = 1 << (shift - 1)
    E = G - np.diag(np.diag(G))
    hi = (E + half) >> shift                         # floor((E + 2^(s-1)) / 2^s)
    lo = E - (hi << shift)
    assert int(np.abs(lo).max(initial=0)) <= half and N * N * half * half < (1 << 63)
    hi8 = hi.astype(np.int8)
    rs2 = np.abs(_int_gram(hi8.astype(np.int64))).sum(axis=1)
    return dict(Ds=Ds, G=G, rs1=rs1, shift=shift, E=E, hi=hi, lo=lo, lo_sumsq=int((lo * lo).sum()), maxdiag=int(np.diag(G).max(initial=0)),
                overflow=int(bool((hi > 127).any() or (hi < -128).any())), hi8=hi8, rs2=rs2)


def restate_python(d, n_pad):
    """The same numbers for the live part as a plain triple loop in Python ints (tests/test_lastdigit_exact_host.py, small n)."""
    N = d.shape[0]
    Ds = [[int(d[min(i, j)][max(i, j)]) if i != j else 0 for j in range(N)] for i in range(N)]
    G = [[sum(Ds[i][k] * Ds[k][j] for k in range(N)) for j in range(N)] for i in range(N)]
    shift = gram_shift(n_pad)
    half = 1 << (shift - 1)
    hi = [[0 if i == j else (G[i][j] + half) // (1 << shift) for j in range(N)] for i in range(N)]
    lo = [[0 if i == j else G[i][j] - hi[i][j] * (1 << shift) for j in range(N)] for i in range(N)]
    wrap = lambda x: (x + 128) % 256 - 128
    h8 = [[wrap(x) for x in row] for row in hi]
    G2 = [[sum(h8[i][k] * h8[k][j] for k in range(N)) for j in range(N)] for i in range(N)]
    return dict(Ds=Ds, G=G, rs1=[sum(abs(x) for x in row) for row in G], hi=hi, lo=lo, lo_sumsq=sum(x * x for row in lo for x in row),
                maxdiag=max([G[i][i] for i in range(N)] + [0]), overflow=int(any(x > 127 or x < -128 for row in hi for x in row)),
                rs2=[sum(abs(x) for x in row) for row in G2])


def bounds(R, n_pad, unit):
    """(H1, H2): |digit error of marker i| <= H q2_i.  H1 from Gershgorin's row sums of |Ds Ds|; H2 from lambda_max(G) <= max G_jj +
    2^s ||E_hi||_2 + ||E_lo||_F, 0 where an entry of E_hi left int8 (no bound).  unit = 2^(e + 2 - 8 S_wc), the weight of the last digit."""
    pad = 0.5 * (n_pad - 1)
    H1 = 0.5 * unit * (np.sqrt(float(R["rs1"].max())) + pad)
    H2 = 0.0
    if not R["overflow"]:
        normsq = float(R["maxdiag"]) + 2.0 ** R["shift"] * np.sqrt(float(R["rs2"].max())) + np.sqrt(float(R["lo_sumsq"]))
        H2 = 0.5 * unit * (np.sqrt(normsq) + pad)
    return H1, H2


def worst_case_count(n_pad, e, half_sumdiag, budget=BUDGET, tight=TIGHT, w_err=0.0):
    """k_vara_prep: (S_wc, the budget in force without the spectral bound)."""
    wc = lambda c: float(n_pad) ** 2 * 2.0 ** (e + 1 - 8 * c) + w_err * n_pad
    S_wc = next((c for c in range(3, 8) if wc(c) <= budget * half_sumdiag), 7)
    return S_wc, (tight if wc(S_wc) <= tight * half_sumdiag else budget)


def decide(S_wc, H1, H2f, half_sumdiag, n_pad, in_force, budget=BUDGET, tight=TIGHT, w_err=0.0, smax=SMAX):
    """k_spectral_decide's order of decisions: the tight budget first (level 1, then level 2), then the default (level 1's bound, then level
    2's).  H2f: a function returning H2, called only where level 2 runs (a spare slot for E_hi: S_wc < smax - 1).
    -> (level that takes the digit off or 0, H, budget in force, whether level 2 ran)."""
    ok = lambda H, b: H > 0.0 and (H + w_err) * n_pad <= b * half_sumdiag
    if S_wc >= smax:
        return 0, 0.0, in_force, False
    if ok(H1, tight):
        return 1, H1, tight, False
    if S_wc >= smax - 1:
        return (1, H1, budget, False) if ok(H1, budget) else (0, 0.0, in_force, False)
    H2 = H2f()
    if ok(H2, tight):
        return 2, H2, tight, True
    if ok(H1, budget):
        return 1, H1, budget, True
    if ok(H2, budget):
        return 2, H2, budget, True
    return 0, 0.0, in_force, True


def scale_exp(mx):
    """w_scale_exp: max |Wu| < 2^e, or < 1.96 x 2^e when the mantissa leaves room."""
    f, e = np.frexp(mx)
    return int(e) - (1 if f <= 0.98 else 0)


def host_decision(Wu, n_pad, budget=BUDGET, tight=TIGHT, w_err=0.0):
    """The library's digit rule restated on the host from the folded W (the tight budget is tried first, at both levels, then the default):
    (worst-case digit count, level of the spectral bound that takes one off or 0, H, budget in force)."""
    off = np.triu(np.asarray(Wu, dtype=np.float64), 1)
    e = scale_exp(np.abs(off).max())
    half_sumdiag = 0.5 * np.abs(np.diag(Wu)).sum()
    S_wc, in_force = worst_case_count(n_pad, e, half_sumdiag, budget, tight, w_err)
    Q = np.rint(np.ldexp(off, 8 * S_wc - (e + 2)))
    d = (np.mod(Q + 128, 256) - 128).astype(np.int64)
    R = restate(d, max(n_pad, d.shape[0]))
    unit = 2.0 ** (e + 2 - 8 * S_wc)
    H1 = bounds(R, n_pad, unit)[0]
    level, H, b, _ = decide(S_wc, H1, lambda: bounds(R, n_pad, unit)[1], half_sumdiag, n_pad, in_force, budget, tight, w_err)
    return S_wc, level, H, b


# ---- the operand builder ------------------------------------------------------------------------------------------------------------
STATES = ("l1", "l2", "l1_default", "none", "ovf_l1", "ovf_none")
# l1: level 1 takes the digit at once (tight budget); l2: level 1 declines, level 2 takes it (tight); l1_default: level 2 runs and
# declines, level 1's bound passes at the default budget; none: both run, nobody passes; ovf_l1 / ovf_none: an entry of E_hi outside int8
# (no level-2 bound) with level 1's bound passing the default budget but not the tight one / passing neither.


def edge_targets(shift, plant):
    """Values of G_jk to plant: {name: value}.  hi = floor((v + 2^(s-1)) / 2^s), lo = v - 2^s hi.  plant: "edge" (inside int8, at its ends
    and at both ends of lo), "overflow" (hi = 128 and -129), "overflow+" / "overflow-" (one of them alone: each side must raise the flag)."""
    half, one = 1 << (shift - 1), 1 << shift
    if plant != "edge":
        over = {"hi=128": 127 * one + half, "hi=-129": -128 * one - half - 1}
        return {k: v for k, v in over.items() if plant == "overflow" or (plant == "overflow+") == (v > 0)}
    return {"hi=127,lo=-half": 127 * one - half, "hi=127,lo=half-1": 127 * one + half - 1, "hi=-128,lo=half-1": -128 * one + half - 1,
            "hi=-128,lo=-half": -128 * one - half}


def _solve_products(v):
    """(alpha, beta), entries in [0, 127], with sum alpha_i beta_i = |v|."""
    t, r = divmod(abs(int(v)), 127 * 127)
    q, p = divmod(r, 127)
    al, be = [127] * t, [127] * t
    if q:
        al.append(127), be.append(q)
    if p:
        al.append(p), be.append(1)
    assert sum(x * y for x, y in zip(al, be)) == abs(int(v))
    return np.array(al, dtype=np.int64), np.array(be, dtype=np.int64)


def plant_positions(n):
    """Three row pairs (j, k), j < k, per target: both rows in the first diagonal tile, both in the last diagonal tile, and one in each
    (an off-diagonal tile: the mirror store carries (k, j)).  G is symmetric, so a pair inside a diagonal tile is met below AND above the
    diagonal.  Rows next to the 32- and 128-row edges of the MFMA blocks and wave halves."""
    assert n > 256 + 16
    last = (n - 1) // 256 * 256
    room = n - last
    return {"diag0": [(31, 128), (127, 160), (0, 255), (96, 33)], "diagL": [(last + 1, last + room - 1), (last, last + 31), (last + 5, last + 32), (last + 9, last + 40)],
            "off": [(32, last + 2), (129, last + 33), (254, last + 3), (63, last + room - 2)]}


def build_case(n, L, S_wc=4, state=None, diag_scale=None, quiet=0, plant=None, loud_row=None, adversarial=0, seed=0, budget=BUDGET,
               tight=TIGHT):
    """-> the dict of exact_scan.build_case (Mt8, S, V, ahat, X, log2u, s, n, L, pairs, probes, zero, plus, minus, dup, max_pair) plus
    n_pad, S_wc, d (last digits above the diagonal), R (restate), H1, H2, sumdiag, decision (level, H, budget, level 2 ran), quiet
    (individuals), quiet_rows / adv_rows (markers), planted {name: [(j, k), ...]}.
    state: one of STATES, the magnitude of the diagonal is solved for; or diag_scale: the magnitude itself.  plant: None, "edge",
    "overflow", "overflow+" or "overflow-" (edge_targets).  loud_row: that row's digits are +-127.  quiet: how many quiet individuals (and as many markers on them)."""
    log2u = LOG2U_OF_SLICES[S_wc]
    sh = -log2u
    n_pad = pad256(n)
    rng = np.random.default_rng(7000003 * n + 1013 * L + 31 * S_wc + 7919 * seed + (0 if loud_row is None else 101 * (loud_row + 1)))
    iu = np.triu_indices(n, 1)
    max_pair = (n // 2, n // 2 + 1)
    h = np.zeros((n, n), dtype=np.int64)
    d = np.zeros((n, n), dtype=np.int64)
    h[iu] = rng.integers(-(1 << 13), 1 << 13, size=iu[0].size)           # |256 h + d| < 2^22: the three lowest digits
    d[iu] = rng.integers(-128, 128, size=iu[0].size)
    reserved = set(max_pair) | {0}
    if loud_row is not None:
        reserved.add(loud_row)
        sg = rng.choice(np.array([-127, 127]), size=n)
        d[loud_row, loud_row + 1:] = sg[loud_row + 1:]
        d[:loud_row, loud_row] = sg[:loud_row]
    planted = {}
    if plant:
        targets = edge_targets(gram_shift(n_pad), plant)
        pos = plant_positions(n)
        rows = sorted({r for lst in pos.values() for p in lst for r in p})
        assert not (set(rows) & set(max_pair))
        reserved |= set(rows)
        d[rows, :] = 0
        d[:, rows] = 0
        cols = np.array([c for c in range(n) if c not in reserved])
        for t, (name, v) in enumerate(sorted(targets.items())):
            planted[name] = []
            for place in ("diag0", "diagL", "off"):
                j, k = sorted(pos[place][t])
                al, be = _solve_products(v)
                assert al.size <= cols.size, "not enough columns for the common support"
                C = rng.choice(cols, size=al.size, replace=False)
                sg = rng.choice(np.array([-1, 1]), size=al.size)
                for c, x, y in zip(C, sg * al, sg * be * (1 if v >= 0 else -1)):
                    d[min(j, c), max(j, c)] = x
                    d[min(k, c), max(k, c)] = y
                planted[name].append((j, k))
    Q = np.array([], dtype=np.int64)
    if quiet:
        free = np.array([c for c in range(n) if c not in reserved])
        Q = np.sort(free[np.linspace(0, free.size - 1, quiet).astype(np.int64)])
        assert np.unique(Q).size == quiet
        for m in (h, d):
            m[Q, :] = 0
            m[:, Q] = 0
    h = np.triu(h, 1)
    d = np.triu(d, 1)
    fix = (d == -128) & (h % 2 != 0)
    h[fix] += 1     # X = 256 h - 128 is a tie of rint(X / 256); the balanced digit -128 leaves h, and round-half-even does for an even h
    X = 256 * h + d
    X[max_pair] = ex.MAXOFF << sh                                         # 2^22 - 1 in absolute value: e = 23; its low byte is 0
    d = np.triu(balanced_low_byte(X), 1)
    R = restate(d, n_pad)
    unit = 2.0 ** (E_SCALE + 2 - 8 * S_wc)
    H1, H2 = bounds(R, n_pad, unit)
    for name, v in (edge_targets(R["shift"], plant).items() if plant else ()):
        for j, k in planted[name]:
            assert R["G"][j, k] == v == R["G"][k, j], (name, j, k, R["G"][j, k], v)
    if plant:
        assert R["overflow"] == (0 if plant == "edge" else 1)
        ends = {"edge": (127, -128), "overflow": (128, -129), "overflow+": (128, None), "overflow-": (None, -129)}[plant]
        assert ends[0] in (None, R["hi"].max()) and ends[1] in (None, R["hi"].min())
        assert -130 < R["hi"].min() and R["hi"].max() < 129             # one step outside int8, on the planted side(s) only
        assert plant != "overflow+" or R["hi"].min() >= -128
        assert plant != "overflow-" or R["hi"].max() <= 127
    if loud_row is not None:
        top = np.sort(R["rs1"])[-2:]
        assert int(np.argmax(R["rs1"])) == loud_row and top[1] - top[0] >= 2
    # the diagonal: an integer strictly above its row's |.| sum, at least the chosen magnitude; sum_k W_kk then decides the state
    X = X + X.T
    dom = -(-np.abs(X).sum(axis=1) >> sh) + 1 + rng.integers(0, 5, size=n)
    live = np.ones(n, dtype=bool)
    live[Q] = False
    sum_for = lambda m, wq: int(np.maximum(dom[live], m).sum()) + wq * int(Q.size)
    T = lambda H, b: H * n_pad / (0.5 * b)                                # sumdiag from which pass(H, b) holds
    s_min = float(n_pad) ** 2 * 2.0 ** (E_SCALE + 1 - 8 * S_wc) / (0.5 * budget)
    s_max = 256.0 * s_min
    if state is not None:
        assert diag_scale is None and state in STATES
        win = {"l1": (T(H1, tight), s_max), "l2": (T(H2, tight), T(H1, tight)), "l1_default": (T(H1, budget), T(H2, tight) if H2 > 0 else 0.0),
               "none": (s_min, min(T(H1, budget), T(H2, budget) if H2 > 0 else np.inf)), "ovf_l1": (T(H1, budget), T(H1, tight)),
               "ovf_none": (s_min, T(H1, budget))}[state]
        lo_, hi_ = max(win[0], s_min), min(win[1], s_max)
        lo_ = max(lo_, float(sum_for(0, 0)) * 1.0001)
        assert lo_ * 1.02 < hi_, ("no room for state %s" % state, lo_, hi_)
        target = min(np.sqrt(lo_ * hi_), 1.5 * lo_)
        a, b = 0, int(target) + 1
        while a < b:                                                     # the smallest magnitude whose sum reaches the target
            m = (a + b) // 2
            if sum_for(m, 0) >= target:
                b = m
            else:
                a = m + 1
        diag_scale = a
    assert diag_scale is not None
    # W_quiet: 12.5 x (the worst-case weight of one pair on S_wc - 1 digits) / (1.8 x the tight budget), an order of magnitude below
    # H / (1.8 x budget), from where a marker's spectral bound H q2 passes: markers on quiet individuals only fail their budget
    wq = int(12.5 * 128.5 * 0.5 * unit / (FLAG_FACTOR * tight)) if quiet else 0
    D = np.maximum(dom, diag_scale)
    D[Q] = wq
    assert not quiet or 0 < wq < D[live].min()
    X[np.arange(n), np.arange(n)] = D << sh
    sumdiag = int(D.sum())
    S_rule, in_force = worst_case_count(n_pad, E_SCALE, 0.5 * sumdiag, budget, tight)
    decision = decide(S_rule, H1, lambda: H2, 0.5 * sumdiag, n_pad, in_force, budget, tight)
    # markers: random genotypes (zero the commonest), then the adversarial rows, the rows on the quiet individuals, the probes and the
    # special rows at the end of the panel
    Mt8 = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(L, n), p=[0.2, 0.55, 0.25])
    mstar = Mt8[0].copy()
    mstar[0] = 1
    mstar[list(max_pair)] = 0
    mstar[Q] = 0
    Mt8[0] = mstar
    pairs = [p for p in ex.planted_pairs(n) if p != max_pair and not (set(p) & set(Q.tolist()))][:6]
    out = dict(pairs=pairs, probes={}, zero=None, plus=None, minus=None, dup=None, max_pair=max_pair, adv_rows=[], quiet_rows=[])
    tail = adversarial + int(Q.size) + 3 * len(pairs) + 4
    if L >= tail + 8:
        r = L - tail
        if adversarial:
            w, U = np.linalg.eigh(R["Ds"][:n, :n].astype(np.float64))
            order = np.argsort(-np.abs(w))
            for t in range(adversarial):
                vec = U[:, order[t]]
                thr = np.sort(np.abs(vec))[n - n // 3]
                Mt8[r] = np.where(np.abs(vec) >= thr, np.sign(vec), 0).astype(np.int8)
                assert (Mt8[r] == 0).sum() > max((Mt8[r] == 1).sum(), (Mt8[r] == -1).sum())
                out["adv_rows"].append(r)
                r += 1
        for t in range(int(Q.size)):                                     # 2 .. quiet non-zero entries, on quiet individuals only
            k = 2 + (t * (Q.size - 2)) // max(1, Q.size - 1)
            Mt8[r] = 0
            Mt8[r, rng.choice(Q, size=k, replace=False)] = rng.choice(np.array([-1, 1], dtype=np.int8), size=k)
            out["quiet_rows"].append(r)
            r += 1
        for (j, k) in pairs:
            for t, sk in enumerate((1, -1, 0)):
                Mt8[r + t] = 0
                Mt8[r + t, j] = 1
                Mt8[r + t, k] = sk
            out["probes"][(j, k)] = (r, r + 1, r + 2)
            r += 3
        Mt8[r] = 0
        Mt8[r + 1] = 1
        Mt8[r + 2] = -1
        Mt8[r + 3] = mstar
        out.update(zero=r, plus=r + 1, minus=r + 2, dup=(0, r + 3))
    else:
        assert not adversarial and not quiet
    ahat = 8 * mstar.astype(np.int64)
    V = np.ldexp(X.astype(np.float64), log2u)
    assert np.array_equal(np.ldexp(V, sh).astype(np.int64), X)           # V = u X exactly
    out.update(Mt8=np.ascontiguousarray(Mt8), S=np.eye(n), V=V, ahat=ahat.astype(np.float64), X=X, log2u=log2u, s=1, n=n, L=L, n_pad=n_pad,
               S_wc=S_wc, d=d, R=R, H1=H1, H2=H2, sumdiag=sumdiag, S_rule=S_rule, decision=decision, quiet=Q, planted=planted, state=state,
               diag_scale=int(diag_scale), unit=unit, wq=wq)
    return out


EXPECTED = {"l1": (1, TIGHT, False), "l2": (2, TIGHT, True), "l1_default": (1, BUDGET, True), "none": (0, None, True),
            "ovf_l1": (1, BUDGET, True), "ovf_none": (0, None, True)}


def assert_state(case):
    """The case reaches the state its name says, judged by the restated rule: the worst-case count, the level, the budget, whether level 2 ran."""
    level, H, b, ran2 = case["decision"]
    want = EXPECTED[case["state"]]
    if case["S_wc"] >= SMAX - 1:
        want = (want[0], want[1], False)                                  # no spare slot for E_hi: level 1 alone
    assert case["S_rule"] == case["S_wc"], (case["S_rule"], case["S_wc"])
    assert (level, ran2) == (want[0], want[2]) and (want[1] is None or b == want[1]), (case["state"], case["decision"])
    assert (H > 0.0) == (level > 0)
    if case["state"].startswith("ovf"):
        assert case["R"]["overflow"] == 1 and case["H2"] == 0.0


def expected_header(case):
    """What the header must read after prepare: S, S_sliced, level, budget and the three level-2 fields (zero unless level 2 ran)."""
    level, H, b, ran2 = case["decision"]
    R = case["R"]
    return dict(S=case["S_wc"] - (1 if level else 0), S_sliced=case["S_wc"], level=level, budget=b, spec_try2=0, e=E_SCALE,
                lo_sumsq=R["lo_sumsq"] if ran2 else 0, maxdiag=R["maxdiag"] if ran2 else 0, hi_overflow=R["overflow"] if ran2 else 0)


def recentre(Mt8):
    """k_marker_shift's c per marker: the majority genotype if it is a homozygote, else the commoner homozygote (-1 on a tie), 0 only for a
    marker without homozygotes."""
    M = np.asarray(Mt8)
    neg, pos = (M == -1).sum(axis=1), (M == 1).sum(axis=1)
    zer = M.shape[1] - neg - pos
    c = np.where((neg > zer) & (neg >= pos), -1, np.where((pos > zer) & (pos > neg), 1, np.where((neg | pos) != 0, np.where(neg >= pos, -1, 1), 0)))
    return c.astype(np.int64)


def lastdigit_miss_units(case, c):
    """(sum_{j<k} m'_j m'_k r_jk in units of u, q2 = sum_j m'_j^2) for m' = m - c: what the scan on S_wc - 1 digits misses of each marker, with
    r = exact_scan.digit_residual_units on S_wc - 1 digits (= 2 d, asserted in the host test)."""
    Ms = case["Mt8"].astype(np.int64) - np.asarray(c, dtype=np.int64)[:, None]
    Rr = ex.digit_residual_units(case, case["S_wc"] - 1, E_SCALE)
    return (ex._exact_matmul(Ms, Rr) * Ms).sum(axis=1), (Ms * Ms).sum(axis=1), np.abs(Ms).sum(axis=1)


def extension_flags(raw, l1, q2, H, budget, e, S_used):
    """k_ext_select: the markers whose own bound min(H q2, l1^2 / 2 x 2^(e+1-8S) (1 + 2^-8)) exceeds 1.8 x budget x |vara|, and the ratio of
    the two sides (callers assert that no marker sits at the threshold)."""
    delta = 2.0 ** (e + 1 - 8 * S_used) * (1.0 + 2.0 ** -8)
    l1 = np.asarray(l1, dtype=np.float64)
    b = np.minimum(H * np.asarray(q2, dtype=np.float64), 0.5 * l1 * l1 * delta)
    thr = FLAG_FACTOR * budget * np.abs(raw)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(thr > 0, b / thr, np.where(b > 0, np.inf, 0.0))
    return b > thr, ratio


# ---- the cases of tests/test_gpu_lastdigit_exact.py, pinned by tests/test_lastdigit_exact_host.py -------------------------------------
PREP_L = 256
SHAPES = (200, 300, 700, 1003)
PREP_STATES = ("l2", "l1_default", "none")
LOUD_ROWS = tuple(sorted(set(range(8)) | {32 * k - 1 for k in range(1, 10)} | {32 * k for k in range(1, 10)} | {299}))
SCAN_CASES = {                                                           # name: (n, L, S_wc, state, packed genotype pass)
    "S4-n300": (300, 1000, 4, "l2", True), "S4-n1003": (1003, 1001, 4, "l1_default", False),
    "S5-n300": (300, 1000, 5, "l1_default", False), "S5-n1003": (1003, 1001, 5, "l2", True),
    "S6-n300": (300, 1000, 6, "l1", True)}
_cache = {}


def _cached(key, make):
    if key not in _cache:
        case = make()
        ex.check_exact(case)
        for arr in (case["X"], case["Mt8"], case["d"]):                  # (V goes to torch.as_tensor, which wants a writable array)
            arr.setflags(write=False)
        _cache[key] = case
    return _cache[key]


def prep_case(n, state):
    return _cached(("prep", n, state), lambda: build_case(n, PREP_L, 4, state=state))


def planted_case(n, state, plant=None):
    """state l2: the edge targets without overflow; ovf_l1 / ovf_none: hi = 128 and -129 planted (plant = "overflow+" / "overflow-": one alone)."""
    plant = plant or ("overflow" if state.startswith("ovf") else "edge")
    assert (plant == "edge") == (state == "l2")
    return _cached(("plant", n, state, plant), lambda: build_case(n, PREP_L, 4, state=state, plant=plant))


PLANTED_CASES = (("l2", "edge"), ("ovf_l1", "overflow"), ("ovf_none", "overflow"), ("ovf_l1", "overflow+"), ("ovf_l1", "overflow-"))


def loud_case(r):
    return _cached(("loud", r), lambda: build_case(300, PREP_L, 4, state="l1", loud_row=r))


def scan_case(name):
    n, L, S_wc, state, _ = SCAN_CASES[name]
    return _cached(("scan", name), lambda: build_case(n, L, S_wc, state=state, quiet=32 if S_wc < 6 else 0, adversarial=6))
