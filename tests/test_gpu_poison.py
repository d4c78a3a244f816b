"""Every device-reaching entry point of rcpp_api on poisoned device allocations (EAGLE_HIP_POISON, csrc/eagle_ctx.h).

The library's buffers hold whatever the process left there: a block freed and taken again, a grow-only buffer of the context that an
earlier, larger call filled.  The hook fills every allocation, and every scratch buffer handed out again, with one byte; a kernel or a
host path that reads memory it did not write then sees that byte instead of the zeros of a fresh process.

One case per entry point (CASES).  A case runs its call on a fixed small input and returns what the caller sees: host arrays and the
bytes of the files written.  test_poisoned runs it
  1. with the hook unset on a new context                                                                    -> clean
  2. for each fill byte, hook set, on a new context, AFTER the same call on an input about twice as large in n and L and without
     missing calls (so the grow-only buffers are larger than the case needs and hold live-looking data behind it) -> dirty
and asserts dirty == clean byte for byte, the counters the library exposes included (as differences around the case's call), and dirty
against the truth the family's own GPU test uses, with that test's comparison.  The fill bytes: 0xFF (NaN in fp64 and fp32, -1 in every
integer width, .bed code 3), 0x7F (1.4e306, 127, 2,139,062,143), 0x55 (1.2e103, 1,431,655,765, the .bed missing code in every bit
pair).  test_kept_state_survives: the four things a context keeps between calls are NOT filled -- a second call under 0xFF hits them
and returns clean's bytes.

Shapes: n = 203 / 257 (no multiple of 4, 64, 256; pad256 has two tiles at 257), L = 129 .. 389 (no multiple of 64, 128, 256; two marker
windows of 256 with a short last one), the exact panels of the spectral, mixed-model, set-test and logistic families at their n = 257.
tests/test_poison_host.py holds the table of cases against the public functions of rcpp_api on the CPU."""
import functools
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN

FILLS = (0xFF, 0x7F, 0x55)
HOOK = "EAGLE_HIP_POISON"
HEAD = b"\x6c\x1b\x01"
E2B_HEADER = 64
NA = np.nan

# public functions of rcpp_api that never reach the device (settings, queries of host-side state, argument helpers); every other one
# has a case below (tests/test_poison_host.py::test_every_entry_point_has_a_case)
NOT_DEVICE = {
    "context", "close_all", "device_info", "last_error",                                     # the context itself: every step opens one
    "set_scan_mode", "set_scan_slices", "set_scan_rounding", "set_scan_budget", "set_w_mode", "drop_cache",      # settings of a context
    "prepare_scan",                                                                           # starts an arena only from 4 GiB up
    "last_scan_budget", "last_scan_enforced", "last_w_info", "last_stream_stats", "last_scan_digits", "last_scan_timing",
    "scan_operand_cache_stats", "w8_keep_stats", "view_load_counts", "is_view", "spectral_holds",                # host-side records
    "getRowColumn",                                                                           # reads the file on the host
    "spectral_traits_passes", "settest_csr", "vcf_flags", "roh_params", "roh_blocks", "ibd_params", "ibd_pairs", "mendel_trios",
    "parentage_lists", "tdt_args",                                                            # argument helpers
}

CASES = {}


class Case:
    def __init__(self, name, family, entries, run, truth, small, big):
        self.name, self.family, self.entries, self.run, self.truth, self.small, self.big = name, family, entries, run, truth, small, big


def case(name, family, entries, small, big, truth=None):
    """Registers run(P, out) -> {key: array | bytes | number} as the case `name`; small / big: the panels (keys of PANELS) of the case
    and of the larger call before it; truth(P, res) asserts res against the family's truth."""
    def deco(run):
        assert name not in CASES
        CASES[name] = Case(name, family, tuple(entries), run, truth, small, big)
        return run
    return deco


# ------------------------------------------------------------------------------------------------ panels
ROOT_DIR = None


class Panel:
    """A genotype panel on disk: Mt8 (L, n) int8, its text pair, and a .bed fileset with the missing calls `miss`."""
    def __init__(self, tag, Mt8, miss=None, extra=None):
        from eagleeverything_amd import r_api, synth
        self.tag = tag
        self.Mt8 = np.ascontiguousarray(Mt8, dtype=np.int8)
        self.L, self.n = self.Mt8.shape
        self.dims = (self.n, self.L)
        self.dir = os.path.join(ROOT_DIR, tag)
        os.makedirs(self.dir)
        self.geno = synth.write_geno_pair(self.dir, self.Mt8)
        self.fM, self.fMt = self.geno["asciifileM"], self.geno["asciifileMt"]
        self.miss = np.zeros(self.Mt8.shape, dtype=bool) if miss is None else miss
        self.bed = synth.write_bed(os.path.join(self.dir, "panel"), self.Mt8, missing=self.miss)
        self.codes = r_api.read_bed_codes(self.bed, self.dims)
        self.extra = extra or {}
        for a in (self.Mt8, self.miss, self.codes):
            a.setflags(write=False)

    def rng(self, salt):
        return np.random.default_rng(1000003 * self.n + 1009 * self.L + salt)


def _random_panel(tag, n, L, seed, miss_rate):
    from eagleeverything_amd import synth
    Mt8 = synth.genotypes_marker_major(n, L, seed=seed)
    Mt8[L - 1] = -1                                   # a monomorphic marker
    Mt8[L - 2] = Mt8[0]                               # a duplicate
    Mt8[5] = 0                                        # every call a heterozygote
    miss = None
    if miss_rate > 0:
        rng = np.random.default_rng(seed + 1)
        miss = rng.random((L, n)) < miss_rate
        miss[3, :] = True                             # a marker without any call
        miss[4, :] = False
    return Panel(tag, Mt8, miss)


def _exact_spectral_panel(tag, n, L):
    import exact_spectral as xs
    c = xs.build_case(n, L)
    return Panel(tag, c["Mt8"], extra={"case": c})


def _lmm_panel(tag, name):
    from test_lmm_host import operands
    ops = operands(name)
    return Panel(tag, ops[7], extra={"name": name, "ops": ops})


def _settest_panel(tag, name):
    from test_settest_host import operands
    ops = operands(name)
    return Panel(tag, ops[5], extra={"name": name, "ops": ops})


def _logistic_panel(tag, name):
    import logistic_truth
    Mt8, st, X, firth_rows, t = logistic_truth.golden(name)
    return Panel(tag, Mt8, extra={"name": name, "st": st, "X": X, "firth_rows": firth_rows, "t": t})


def _golden_panel(tag, name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    return Panel(tag, np.ascontiguousarray(g["M8"].T))


PANELS = {
    # small: 2 % missing calls in the .bed file; big: about twice n and L, nothing missing
    "s203": lambda: _random_panel("s203", 203, 389, 11, 0.02),
    "b411": lambda: _random_panel("b411", 411, 777, 12, 0.0),
    "s257": lambda: _random_panel("s257", 257, 389, 13, 0.02),      # pad256(n) = 512: two 256-tiles for the scan and the W engine
    "b515": lambda: _random_panel("b515", 515, 777, 14, 0.0),
    "s203e": lambda: _random_panel("s203e", 203, 129, 15, 0.0),     # all pairs of markers: 8,256
    "b411e": lambda: _random_panel("b411e", 411, 257, 16, 0.0),
    "xs257": lambda: _exact_spectral_panel("xs257", 257, 257),
    "xb515": lambda: _exact_spectral_panel("xb515", 515, 517),
    "lmm257": lambda: _lmm_panel("lmm257", "n257"),
    "lmm1003": lambda: _lmm_panel("lmm1003", "n1003"),
    "set257": lambda: _settest_panel("set257", "n257"),
    "set1003": lambda: _settest_panel("set1003", "n1003"),
    "log257": lambda: _logistic_panel("log257", "n257"),
    "log1003": lambda: _logistic_panel("log1003", "n1003"),
    "e2e": lambda: _golden_panel("e2e", "synth_203x1531"),
    "e2eb": lambda: Panel("e2eb", __import__("eagleeverything_amd.synth", fromlist=["synth"]).genotypes_marker_major(406, 3062, seed=17)),
}


@functools.lru_cache(maxsize=None)
def panel(key):
    return PANELS[key]()


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _sidecar(path):
    """The packed rows of the 2-bit sidecar of a text file (its header carries the text file's mtime), b"" without one."""
    return _read(path + ".e2b")[E2B_HEADER:] if os.path.exists(path + ".e2b") else b""


def _api():
    from eagleeverything_amd import rcpp_api
    return rcpp_api


class env:
    """Environment variables for the length of a with block."""
    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(res, exp, keys=None):
    """== on every key of exp: dtype, shape and values (integer and byte families)."""
    for k in (keys or exp):
        g, w = res[k], exp[k]
        if isinstance(w, (bytes, int, float, str, list, tuple)) or w is None:
            assert g == w, k
        else:
            w = np.asarray(w)
            assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
            assert np.array_equal(g, w, equal_nan=w.dtype.kind == "f"), (k, np.argwhere(g != w)[:5].tolist())


# ------------------------------------------------------------------------------------------------ Gram and scan
def _oracle():
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c


def _scan_operands(P):
    rng = P.rng(1)
    n = P.n
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    S = A @ A.T + np.eye(n)
    V = 0.5 * np.eye(n) - 0.01 * np.outer(A[:, 0], A[:, 0])
    return S, V, rng.standard_normal(n)


def _truth_mmt(sel):
    def truth(P, res):
        ref = _oracle().calculateMMt_rcpp(P.fM, 8.0, 2, sel(P), P.dims)
        assert np.array_equal(res["MMt"], ref)                             # exact integers (smoke())
        if "norm" in res:
            # calcMMt.R:13, MMt / max(MMt) + 0.95 I: one rounding in the quotient, one in the sum
            want = ref / ref.max()
            want[np.diag_indices(P.n)] += 0.95
            assert res["max"] == ref.max()
            np.testing.assert_allclose(res["norm"], want, rtol=4 * 2.0 ** -53, atol=0)
    return truth


@case("calculateMMt_rcpp", "gram", ["calculateMMt_rcpp", "last_mmt_normalised"], "s257", "b515", _truth_mmt(lambda P: NA))
def _(P, out):
    api = _api()
    mmt = api.calculateMMt_rcpp(P.fM, 8.0, 2, NA, P.dims)
    norm, mx = api.last_mmt_normalised(P.n)
    return {"MMt": mmt, "norm": norm, "max": mx}


def _sel_loci(P):
    return np.array([0.0, 7.0, P.L // 2, P.L - 1.0])


@case("calculateMMt_rcpp selected", "gram", ["calculateMMt_rcpp"], "s257", "b515", _truth_mmt(_sel_loci))
def _(P, out):
    return {"MMt": _api().calculateMMt_rcpp(P.fM, 8.0, 2, _sel_loci(P), P.dims)}


def _truth_scan(P, res):
    """smoke()'s bounds: a within 1e-9, vara within 1e-7 (the digit-slice certificate enforces 9e-7 at most), the selected marker."""
    orc = _oracle()
    S, V, ahat = _scan_operands(P)
    exp = orc.calculate_a_and_vara_rcpp(P.fMt, NA, S, V, 8.0, (P.L, P.n), ahat)
    np.testing.assert_allclose(res["a"], exp["a"], rtol=1e-9, atol=1e-12 * np.abs(exp["a"]).max())
    np.testing.assert_allclose(res["vara"], exp["vara"], rtol=1e-7)
    if "argmax" in res:
        _, idx_ref, _ = orc.tsq_argmax(exp["a"], exp["vara"])
        assert int(res["argmax"][0]) == idx_ref
    if "int8" in res:
        assert res["int8"] == 1, "the W engine declined"


def _scan(P, mode, w_mode=None):
    api = _api()
    api.set_scan_mode(mode)
    if w_mode is not None:
        api.set_w_mode(w_mode)
    S, V, ahat = _scan_operands(P)
    res = api.calculate_a_and_vara_rcpp(P.fMt, NA, S, V, 8.0, (P.L, P.n), ahat)
    out = {"a": res["a"], "vara": res["vara"], "argmax": np.array(api.last_scan_argmax(), dtype=np.float64),
           "certificate": np.array(api.last_scan_certificate(), dtype=np.int64), "digits": np.array(api.last_scan_digits(), dtype=np.float64)}
    if w_mode is not None:
        out["int8"] = api.last_w_info()["int8"]
    return out


@case("calculate_a_and_vara_rcpp mode 0", "scan", ["calculate_a_and_vara_rcpp", "last_scan_argmax", "last_scan_certificate"], "s257", "b515",
      _truth_scan)
def _(P, out):
    return _scan(P, 0)


@case("calculate_a_and_vara_rcpp mode 1", "scan", ["calculate_a_and_vara_rcpp", "last_scan_argmax", "last_scan_certificate"], "s257", "b515",
      _truth_scan)
def _(P, out):
    return _scan(P, 1)


@case("calculate_a_and_vara_rcpp w_mode 2", "scan", ["calculate_a_and_vara_rcpp"], "s257", "b515", _truth_scan)
def _(P, out):
    return _scan(P, 1, w_mode=2)


@case("scan_with_W", "scan", ["scan_with_W"], "s257", "b515", _truth_scan)
def _(P, out):
    S, V, ahat = _scan_operands(P)
    res = _api().scan_with_W(P.fMt, NA, S @ V @ S, S @ ahat, 8.0, (P.L, P.n))
    return {"a": res["a"], "vara": res["vara"]}


def _reduced_operands(P):
    rng = P.rng(2)
    B = rng.standard_normal((P.n, P.n)) / np.sqrt(P.n)
    return 0.7, B @ B.T + 0.1 * np.eye(P.n), rng.standard_normal(P.n)


def _truth_reduced(P, res):
    varG, Pm, y = _reduced_operands(P)
    ref = _oracle().calculate_reduced_a_rcpp(P.fMt, varG, Pm, y, 8.0, P.dims, NA)
    np.testing.assert_allclose(res["ar"], ref, rtol=1e-9, atol=1e-12 * np.abs(ref).max())        # as `a` in smoke(): the same product


@case("calculate_reduced_a_rcpp", "scan", ["calculate_reduced_a_rcpp"], "s257", "b515", _truth_reduced)
def _(P, out):
    varG, Pm, y = _reduced_operands(P)
    return {"ar": _api().calculate_reduced_a_rcpp(P.fMt, varG, Pm, y, 8.0, P.dims, NA)}


def _truth_extract(P, res):
    orc = _oracle()
    for k, c in enumerate((0, P.L // 2 + 3, P.L - 1)):
        assert np.array_equal(res["geno%d" % k], orc.extract_geno_rcpp(P.fM, 8.0, c, P.dims))
        assert np.array_equal(res["geno%d" % k], P.Mt8[c].astype(np.int32))
    assert np.array_equal(res["rb"], orc.ReadBlock(P.fMt, P.L - 5, P.n, 5))
    assert np.array_equal(res["rbM"], orc.ReadBlock(P.fM, P.n - 2, P.L, 2))


@case("extract_geno_rcpp and ReadBlock", "scan", ["extract_geno_rcpp", "ReadBlock"], "s257", "b515", _truth_extract)
def _(P, out):
    api = _api()
    res = {"geno%d" % k: api.extract_geno_rcpp(P.fM, 8.0, c, P.dims) for k, c in enumerate((0, P.L // 2 + 3, P.L - 1))}
    res["rb"] = api.ReadBlock(P.fMt, P.L - 5, P.n, 5)
    res["rbM"] = api.ReadBlock(P.fM, P.n - 2, P.L, 2)
    return res


# ------------------------------------------------------------------------------------------------ spectral (exact dyadic truth)
def _xs_prepare(P, mode=1):
    api = _api()
    c = P.extra["case"]
    api.set_scan_mode(mode)
    try:
        api.spectral_prepare(P.fMt, (c["L"], c["n"]), c["U"], 8.0)
    finally:
        api.set_scan_mode(1)
    return api, c


def _xs_single(c, p, sel=()):
    import exact_spectral as xs
    op = xs.single_op(c, p)
    xs.check_exact(c, op)
    return op, xs.truth(c, op, sel=sel)


def _truth_z(P, res):
    import exact_spectral as xs
    xs.assert_z(res["Z"].T, P.extra["case"], "Z")


def _prepare_case(mode):
    def run(P, out):
        api, c = _xs_prepare(P, mode)
        return {"Z": api.spectral_rows(np.arange(c["L"]))}
    return run


case("spectral_prepare mode 1", "spectral", ["spectral_prepare", "spectral_rows"], "xs257", "xb515", _truth_z)(_prepare_case(1))
case("spectral_prepare mode 0", "spectral", ["spectral_prepare", "spectral_rows"], "xs257", "xb515", _truth_z)(_prepare_case(0))


def _truth_rows(P, res):
    c = P.extra["case"]
    idx = np.arange(c["L"])[::-7]
    assert np.array_equal(res["rows"].T, c["Z"][idx])


@case("spectral_rows", "spectral", ["spectral_rows"], "xs257", "xb515", _truth_rows)
def _(P, out):
    api, c = _xs_prepare(P)
    return {"rows": api.spectral_rows(np.arange(c["L"])[::-7].copy())}


def _truth_xs_scan(P, res):
    import exact_spectral as xs
    c = P.extra["case"]
    for p in xs.single_ps(c):
        op, tr = _xs_single(c, p)
        xs.assert_scan(res["a%d" % p], res["vara%d" % p], tr, "p=%d" % p)
        xs.assert_planted(res["a%d" % p], res["vara%d" % p], c, op, tr, "p=%d" % p)
    sel = tuple(sorted({0, c["L"] // 2, c["L"] - 1}))
    p = xs.single_ps(c)[0]
    _, trm = _xs_single(c, p, sel)
    xs.assert_scan(res["am"], res["varam"], trm, "masked")


def _xs_scan_case(weights):
    def run(P, out):
        import exact_spectral as xs
        api, c = _xs_prepare(P)
        L = c["L"]
        res = {}
        sel = np.array(sorted({0, L // 2, L - 1}), dtype=np.float64)
        for k, p in enumerate(xs.single_ps(c)):
            op = xs.single_op(c, p)
            UtX, Uty = op["X"].astype(np.float64), op["y"].astype(np.float64)
            if weights:
                r = api.spectral_scan_weights(op["d"], op["d"] * Uty, op["d"][:, None] * UtX, op["C"], op["c1"], op["varG"], L)
            else:
                r = api.spectral_scan(c["lam"], UtX, Uty, op["varE"], op["varG"], L)
            res["a%d" % p], res["vara%d" % p] = r["a"], r["vara"]
            if k == 0:
                if weights:
                    rm = api.spectral_scan_weights(op["d"], op["d"] * Uty, op["d"][:, None] * UtX, op["C"], op["c1"], op["varG"], L, selected_loci=sel)
                else:
                    rm = api.spectral_scan(c["lam"], UtX, Uty, op["varE"], op["varG"], L, selected_loci=sel)
                res["am"], res["varam"] = rm["a"], rm["vara"]
        return res
    return run


case("spectral_scan", "spectral", ["spectral_scan"], "xs257", "xb515", _truth_xs_scan)(_xs_scan_case(False))
case("spectral_scan_weights", "spectral", ["spectral_scan_weights"], "xs257", "xb515", _truth_xs_scan)(_xs_scan_case(True))


def _trait_ops(c, k):
    import exact_spectral as xs
    plist, widths = xs.TRAIT_LISTS[k]
    return plist, [xs.trait_op(c, t, p) for t, p in enumerate(plist)]


def _truth_traits(P, res):
    import exact_spectral as xs
    c = P.extra["case"]
    for k in (0, 1):
        plist, ops = _trait_ops(c, k)
        for t, op in enumerate(ops):
            xs.check_exact(c, op)
            tr = xs.truth(c, op)
            what = "list %d trait %d" % (k, t)
            xs.assert_scan(res["a%d" % k][:, t], res["vara%d" % k][:, t], tr, what)
            xs.assert_argmax(res["index%d" % k][t], res["tsqmax%d" % k][t], tr, what)


@case("spectral_scan_traits", "spectral", ["spectral_scan_traits"], "xs257", "xb515", _truth_traits)
def _(P, out):
    api, c = _xs_prepare(P)
    res = {}
    for k in (0, 1):                                   # 20 traits of p = 4 (groups of 8 and 2 tiles), 5 traits of p = 31, 31, 31, 31, 20
        plist, ops = _trait_ops(c, k)
        UtX = [op["X"].astype(np.float64) for op in ops]
        UtY = np.column_stack([op["y"] for op in ops]).astype(np.float64)
        r = api.spectral_scan_traits(c["lam"], UtX, UtY, [op["varE"] for op in ops], [op["varG"] for op in ops], c["L"], full=True)
        for key in ("index", "tsqmax", "a", "vara"):
            res["%s%d" % (key, k)] = r[key]
    return res


def _lmm_prepare(P):
    api = _api()
    ops = P.extra["ops"]
    api.set_scan_mode(0)                                # the truth's bounds carry fp64 rounding of Z (tests/test_gpu_lmm.py)
    try:
        api.spectral_prepare(P.fMt, (P.L, P.n), ops[1], 8.0)
    finally:
        api.set_scan_mode(1)
    return api, ops


def _lmm_case(method):
    def run(P, out):
        from test_lmm_host import TOL
        api, (lam, U, UtX, Uty, Z, th_r, th_m, Mt8, X, y) = _lmm_prepare(P)
        stat, info = api.spectral_lmm(lam, UtX, Uty, reml=method == "reml", theta0=th_r if method == "reml" else th_m, tol=TOL, n_markers=P.L)
        rev = np.arange(P.L)[::-1].copy()
        s2, i2 = api.spectral_lmm(lam, UtX, Uty, reml=method == "reml", theta0=th_r if method == "reml" else th_m, tol=TOL, idx=rev)
        return {"stat": stat, "info": info, "stat_rev": s2, "info_rev": i2}

    def truth(P, res):
        from test_lmm_host import assert_meets_truth
        assert_meets_truth(P.extra["name"], method, res["stat"], res["info"], P.n)
        assert res["stat"][::-1].tobytes() == res["stat_rev"].tobytes() and np.array_equal(res["info"][::-1], res["info_rev"])
    return run, truth


for _m in ("reml", "ml"):
    _run, _truth = _lmm_case(_m)
    case("spectral_lmm " + _m, "lmm", ["spectral_lmm"], "lmm257", "lmm1003", _truth)(_run)


def _truth_settest(P, res):
    from test_settest_host import assert_meets_truth
    k = len(P.extra["ops"][8])
    assert_meets_truth(P.extra["name"], {"stat": res["stat"], "info": res["info"], "score": [res["score%d" % o] for o in range(k)],
                                          "cov": [res["cov%d" % o] for o in range(k)]})


@case("spectral_settest", "lmm", ["spectral_settest"], "set257", "set1003", _truth_settest)
def _(P, out):
    import settest_truth as T
    api = _api()
    lam, U, UtX, Uty, Z, Mt8, X, y, st, om = P.extra["ops"]
    api.set_scan_mode(0)
    try:
        api.spectral_prepare(P.fMt, (P.L, P.n), U, 8.0)
    finally:
        api.set_scan_mode(1)
    r = api.spectral_settest(lam, UtX, Uty, T.VAR_E, T.VAR_G, st, om, scores=True, cov=True)
    res = {"stat": r["stat"], "info": r["info"]}
    for o in range(len(st)):
        res["score%d" % o], res["cov%d" % o] = r["score"][o], r["cov"][o]
    return res


# ------------------------------------------------------------------------------------------------ ingestion
def _table(path, M8):
    """The genotype table ReadMarker(type="text") reads: one line per individual, '0' '1' '2' separated by blanks."""
    digits = (np.asarray(M8) + 1).astype(np.uint8) + ord("0")
    buf = np.full((digits.shape[0], 2 * digits.shape[1]), ord(" "), dtype=np.uint8)
    buf[:, 0::2] = digits
    buf[:, -1] = ord("\n")
    with open(path, "wb") as f:
        f.write(buf.tobytes())
    return path


def _truth_createM(P, res):
    assert res["ok"] and res["M"] == _read(P.fM)


@case("createM_ASCII_rcpp", "ingest", ["createM_ASCII_rcpp"], "s203", "b411", _truth_createM)
def _(P, out):
    src = _table(os.path.join(out, "table.txt"), P.Mt8.T)
    fM = os.path.join(out, "M.ascii")
    ok = _api().createM_ASCII_rcpp(src, fM, "text", 0, 1, 2, 8.0, P.dims)
    return {"ok": bool(ok), "M": _read(fM), "M.e2b": _sidecar(fM)}


def _truth_createMt(P, res):
    assert res["Mt"] == _read(P.fMt)


@case("createMt_ASCII_rcpp", "ingest", ["createMt_ASCII_rcpp"], "s203", "b411", _truth_createMt)
def _(P, out):
    fM, fMt = os.path.join(out, "M.ascii"), os.path.join(out, "Mt.ascii")
    shutil.copy(P.fM, fM)
    _api().createMt_ASCII_rcpp(fM, fMt, "text", 8.0, P.dims)
    return {"Mt": _read(fMt), "Mt.e2b": _sidecar(fMt)}


def _truth_from_bed(P, res):
    het = np.where(P.miss, 0, P.Mt8).astype(np.int8)             # a missing genotype is coded as a heterozygote
    text = lambda G: (np.concatenate([(G + 1 + ord("0")).astype(np.uint8), np.full((G.shape[0], 1), ord("\n"), dtype=np.uint8)], axis=1)).tobytes()
    assert res["n_missing"] == int(P.miss.sum())
    assert res["Mt"] == text(het) and res["M"] == text(np.ascontiguousarray(het.T))


@case("create_ascii_from_bed", "ingest", ["create_ascii_from_bed"], "s203", "b411", _truth_from_bed)
def _(P, out):
    fM, fMt = os.path.join(out, "M.ascii"), os.path.join(out, "Mt.ascii")
    nm = _api().create_ascii_from_bed(P.bed, fM, fMt, 8.0, P.dims)
    return {"n_missing": nm, "M": _read(fM), "Mt": _read(fMt), "M.e2b": _sidecar(fM), "Mt.e2b": _sidecar(fMt)}


@functools.lru_cache(maxsize=None)
def _vcf_text(n):
    from test_gpu_vcf import make_vcf
    return make_vcf(n, seed=n, lines=60 if n < 300 else 120)


def _vcf_case(chunk):
    def run(P, out):
        src = os.path.join(out, "in.vcf")
        with open(src, "wb") as f:
            f.write(_vcf_text(P.n))
        r = _api().vcf_to_bed(src, os.path.join(out, "panel"), chunk_bytes=chunk)
        return {"dims": list(r["dims"]), "counts": tuple(sorted(r["counts"].items())), "bed": _read(r["bed"]), "bim": _read(r["bim"]),
                "fam": _read(r["fam"])}

    def truth(P, res):
        from eagleeverything_amd import r_api
        bed, bim, fam, dims, counts = r_api.vcf_to_bed_host(_vcf_text(P.n))
        assert res["dims"] == list(dims) and dict(res["counts"]) == counts
        assert res["bed"] == bed and res["bim"].decode("latin-1") == bim and res["fam"].decode("latin-1") == fam
    return run, truth


for _c in (1, 0):
    _run, _truth = _vcf_case(_c)
    case("vcf_to_bed chunk_bytes %d" % _c, "ingest", ["vcf_to_bed"], "s203", "b411", _truth)(_run)


def _keep(P):
    return np.flatnonzero(np.arange(P.L) % 3 != 1)


def _truth_filter(P, res):
    from eagleeverything_amd import synth
    keep = _keep(P)
    d = os.path.join(P.dir, "filter_truth")
    os.makedirs(d, exist_ok=True)
    g = synth.write_geno_pair(d, P.Mt8[keep])
    assert res["dims"] == [P.n, keep.size]
    assert res["M"] == _read(g["asciifileM"]) and res["Mt"] == _read(g["asciifileMt"])


@case("filter_markers", "ingest", ["filter_markers"], "s203", "b411", _truth_filter)
def _(P, out):
    oM, oMt = os.path.join(out, "fM.ascii"), os.path.join(out, "fMt.ascii")
    nd = _api().filter_markers(P.fM, P.fMt, P.dims, _keep(P), oM, oMt)
    return {"dims": list(nd), "M": _read(oM), "Mt": _read(oMt), "M.e2b": _sidecar(oM), "Mt.e2b": _sidecar(oMt)}


def _truth_view(P, res):
    from test_gpu_marker_qc import np_counts
    na = np.array([3, P.n - 1, 77])
    kept = np.setdiff1d(np.arange(P.n), na)
    assert res["dims"] == [P.n - 3, P.L]
    assert np.array_equal(res["counts"], np_counts(P.Mt8.T[kept]))


@case("ReshapeM_rcpp view", "ingest", ["ReshapeM_rcpp"], "s203", "b411", _truth_view)
def _(P, out):
    api = _api()
    nd = api.ReshapeM_rcpp(P.fM, P.fMt, [3, P.n - 1, 77], P.dims, view=True)
    return {"dims": list(nd), "counts": api.marker_counts(P.fMt + "tmp", nd)}


# ------------------------------------------------------------------------------------------------ counts and QC
def _labels(P, K=5):
    return (P.rng(3).integers(-1, K, size=P.n)).astype(np.int64)


def _np_bed_counts(codes, axis):
    return np.stack([np.sum(codes == v, axis=axis) for v in (0, 2, 3, 1)], axis=1).astype(np.int32)


def _counts_truth(fn):
    return lambda P, res: _same(res, fn(P))


@case("marker_counts", "counts", ["marker_counts"], "s203", "b411",
      _counts_truth(lambda P: {"counts": __import__("test_gpu_marker_qc").np_counts(P.Mt8.T)}))
def _(P, out):
    return {"counts": _api().marker_counts(P.fMt, P.dims)}


@case("bed_marker_counts", "counts", ["bed_marker_counts"], "s203", "b411", _counts_truth(lambda P: {"counts": _np_bed_counts(P.codes, 1)}))
def _(P, out):
    return {"counts": _api().bed_marker_counts(P.bed, P.dims)}


@case("sample_counts", "counts", ["sample_counts"], "s203", "b411",
      _counts_truth(lambda P: {"counts": __import__("test_gpu_sample_qc").np_sample_counts(P.Mt8.T)}))
def _(P, out):
    return {"counts": _api().sample_counts(P.fM, P.dims)}


@case("bed_sample_counts", "counts", ["bed_sample_counts"], "s203", "b411", _counts_truth(lambda P: {"counts": _np_bed_counts(P.codes, 0)}))
def _(P, out):
    return {"counts": _api().bed_sample_counts(P.bed, P.dims)}


def _r_api():
    from eagleeverything_amd import r_api
    return r_api


@case("group_counts", "counts", ["group_counts"], "s203", "b411",
      _counts_truth(lambda P: {"counts": _r_api().group_counts_host(P.Mt8, _labels(P), 5)}))
def _(P, out):
    return {"counts": _api().group_counts(P.fMt, P.dims, _labels(P), 5)}


@case("bed_group_counts", "counts", ["bed_group_counts"], "s203", "b411",
      _counts_truth(lambda P: {"counts": _r_api().bed_group_counts_host(P.codes, _labels(P), 5)}))
def _(P, out):
    return {"counts": _api().bed_group_counts(P.bed, P.dims, _labels(P), 5)}


def _fisher_tables(P):
    return P.rng(4).integers(0, 60, size=(P.L, 4)).astype(np.int32)


def _truth_exact_tests(P, res):
    from test_gpu_sample_qc import py_hwe_rows
    assert res["hwe"].tobytes() == py_hwe_rows(_np_bed_counts(P.codes, 1)).tobytes()
    assert res["fisher"].tobytes() == _r_api().fisher_2x2_host(_fisher_tables(P)).tobytes()


@case("hwe_exact and fisher_2x2", "counts", ["hwe_exact", "fisher_2x2"], "s203", "b411", _truth_exact_tests)
def _(P, out):
    api = _api()
    return {"hwe": api.hwe_exact(_np_bed_counts(P.codes, 1)), "fisher": api.fisher_2x2(_fisher_tables(P))}


# ------------------------------------------------------------------------------------------------ relatedness and imputation
@functools.lru_cache(maxsize=None)
def _ibs_truth(key):
    from test_gpu_sample_qc import np_ibs
    ibs0, hethet = np_ibs(panel(key).Mt8.T)
    return ibs0.astype(np.int32), hethet.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _bed_ibs_truth(key):
    return _r_api().bed_ibs_host(panel(key).codes)


@case("sample_ibs", "related", ["sample_ibs"], "s203", "b411", lambda P, res: _same(res, dict(zip(("ibs0", "hethet"), _ibs_truth(P.tag)))))
def _(P, out):
    ibs0, hethet = _api().sample_ibs(P.fM, P.dims)
    return {"ibs0": ibs0, "hethet": hethet}


_BED_IBS = ("ncalled", "ibs0", "hethet", "hetsum", "dist")


@case("bed_sample_ibs", "related", ["bed_sample_ibs"], "s203", "b411", lambda P, res: _same(res, dict(zip(_BED_IBS, _bed_ibs_truth(P.tag)))))
def _(P, out):
    return dict(zip(_BED_IBS, _api().bed_sample_ibs(P.bed, P.dims)))


def _truth_knn(P, res):
    ibs0, hethet = _ibs_truth(P.tag)
    _same(res, {"nbr": _r_api().knn_rows_host(_r_api().knn_distance(ibs0, hethet), 9)})


@case("knn_rows", "related", ["knn_rows"], "s203", "b411", _truth_knn)
def _(P, out):
    ibs0, hethet = _ibs_truth(P.tag)
    return {"nbr": _api().knn_rows(ibs0, hethet, 9)}


def _truth_knn_dist(P, res):
    _same(res, {"nbr": _r_api().knn_rows_host(_bed_ibs_truth(P.tag)[4], 9)})        # the uint32 matrix as it is


@case("knn_rows_dist", "related", ["knn_rows_dist"], "s203", "b411", _truth_knn_dist)
def _(P, out):
    return {"nbr": _api().knn_rows_dist(_bed_ibs_truth(P.tag)[4], 9)}


def _truth_impute(P, res):
    from test_gpu_impute import table
    rows, counts = _r_api().impute_knn_host(P.codes, table(P.n, 9, P.n), 5, 2)
    assert res["bed"] == HEAD + rows.tobytes()
    _same(res, {"counts": counts})


@case("bed_impute_knn", "related", ["bed_impute_knn"], "s203", "b411", _truth_impute)
def _(P, out):
    from test_gpu_impute import table
    o = os.path.join(out, "imputed.bed")
    counts = _api().bed_impute_knn(P.bed, P.dims, table(P.n, 9, P.n), 5, 2, o)
    return {"counts": counts, "bed": _read(o)}


@functools.lru_cache(maxsize=None)
def _partners(key, l=6):
    P = panel(key)
    rng = P.rng(5)
    pt = np.full((P.L, l), -1, dtype=np.int32)
    for m in range(P.L):
        near = [j for j in range(max(0, m - 5), min(P.L, m + 6)) if j != m]
        pick = rng.permutation(near)[:rng.integers(1, l + 1)]
        pt[m, :pick.size] = pick
    pt[17, :] = -1                                      # no partners: every missing genotype of marker 17 by fallback
    pt[20, :3] = (22, 22, 19)                           # a repeated partner counts twice
    return pt


def _truth_ldknn(P, res):
    rows, counts = _r_api().impute_ldknn_host(P.codes, _partners(P.tag), 5, 2, 2)
    assert res["bed"] == HEAD + rows.tobytes()
    _same(res, {"counts": counts})


@case("bed_impute_ldknn", "related", ["bed_impute_ldknn"], "s203", "b411", _truth_ldknn)
def _(P, out):
    o = os.path.join(out, "ldknn.bed")
    counts = _api().bed_impute_ldknn(P.bed, P.dims, _partners(P.tag), 5, 2, 2, o)
    return {"counts": counts, "bed": _read(o)}


# ------------------------------------------------------------------------------------------------ LD and haplotypes
W = 50
EDGES = [1, 2, 5, 10, 25, 51]


def _truth_ld_window(P, res):
    from test_gpu_ld import np_mask, popcount
    mask = np_mask(P.Mt8.T, W, 0.2)
    _same(res, {"mask": mask})
    assert res["pairs"] == popcount(mask)


@case("ld_window", "ld", ["ld_window"], "s203", "b411", _truth_ld_window)
def _(P, out):
    mask, pairs = _api().ld_window(P.fMt, P.dims, W, 0.2, return_pairs=True)
    return {"mask": mask, "pairs": pairs}


def _loci(P):
    return np.array([0, 5, P.L // 2, P.L - 1, 5])


@case("ld_dots", "ld", ["ld_dots"], "s203", "b411",
      lambda P, res: _same(res, {"dots": (P.Mt8.astype(np.int64) @ P.Mt8[_loci(P)].astype(np.int64).T).astype(np.int32)}))
def _(P, out):
    return {"dots": _api().ld_dots(P.fMt, P.dims, _loci(P))}


@case("ld_partners", "ld", ["ld_partners"], "s203", "b411",
      lambda P, res: _same(res, dict(zip(("partners", "r2"), _r_api().ld_partners_host(P.Mt8, W, 16, 0.05)))))
def _(P, out):
    pt, r2 = _api().ld_partners(P.fMt, P.dims, W, 16, 0.05, return_r2=True)
    return {"partners": pt, "r2": r2}


_LD_STATS = ("U", "cnt", "bin_sum", "bin_pairs")


@case("ld_stats", "ld", ["ld_stats"], "s203", "b411",
      lambda P, res: _same(res, dict(zip(_LD_STATS, _r_api().ld_stats_host(_r_api().ld_band_host(P.Mt8, W), edges=EDGES)))))
def _(P, out):
    return dict(zip(_LD_STATS, _api().ld_stats(P.fMt, P.dims, W, edges=EDGES)))


def _include(P):
    inc = np.ones(P.L, dtype=bool)
    inc[7::11] = False
    return inc


def _truth_bed_ld_window(P, res):
    from test_gpu_ld import popcount
    mask = _r_api().bed_ld_mask_host(P.codes, W, 0.2, include=_include(P), min_overlap=3)
    _same(res, {"mask": mask})
    assert res["pairs"] == popcount(mask)


@case("bed_ld_window", "ld", ["bed_ld_window"], "s203", "b411", _truth_bed_ld_window)
def _(P, out):
    mask, pairs = _api().bed_ld_window(P.bed, P.dims, W, 0.2, include=_include(P), min_overlap=3, return_pairs=True)
    return {"mask": mask, "pairs": pairs}


@case("bed_ld_partners", "ld", ["bed_ld_partners"], "s203", "b411",
      lambda P, res: _same(res, dict(zip(("partners", "r2"), _r_api().bed_ld_partners_host(P.codes, W, 16, 0.05, include=_include(P), min_overlap=3)))))
def _(P, out):
    pt, r2 = _api().bed_ld_partners(P.bed, P.dims, W, 16, 0.05, include=_include(P), min_overlap=3, return_r2=True)
    return {"partners": pt, "r2": r2}


@case("bed_ld_stats", "ld", ["bed_ld_stats"], "s203", "b411",
      lambda P, res: _same(res, dict(zip(_LD_STATS, _r_api().ld_stats_host(_r_api().bed_ld_host(P.codes, W, include=_include(P), min_overlap=3)[6],
                                                                            edges=EDGES)))))
def _(P, out):
    return dict(zip(_LD_STATS, _api().bed_ld_stats(P.bed, P.dims, W, include=_include(P), min_overlap=3, edges=EDGES)))


def _truth_hap_ld(P, res):
    from test_gpu_hapld import same
    same(res, _r_api().hap_ld_host(P.Mt8, 33), "hap_ld")


@case("hap_ld", "ld", ["hap_ld"], "s203e", "b411e", _truth_hap_ld)
def _(P, out):
    return _api().hap_ld(P.fMt, P.dims, 33, bands=True)


# ------------------------------------------------------------------------------------------------ runs, sharing and families
ROH = dict(w=10, win_het=1, win_miss=2, min_snp=8)
IBD = dict(mode=1, min_snp=10, merge_min=4, max_gap=0)


def _chrom(P):
    return (np.arange(P.L) >= P.L // 2 + 3).astype(np.int32)


@case("roh", "runs", ["roh"], "s203", "b411",
      lambda P, res: _same(res, dict(zip(("ind", "seg"), _r_api().roh_host(_r_api().roh_classes_mt8(P.Mt8), chrom=_chrom(P), **ROH)))))
def _(P, out):
    ind, seg = _api().roh(P.fMt, P.dims, chrom=_chrom(P), **ROH)
    return {"ind": ind, "seg": seg}


@case("bed_roh", "runs", ["bed_roh"], "s203", "b411",
      lambda P, res: _same(res, dict(zip(("ind", "seg"), _r_api().roh_host(_r_api().roh_classes_bed(P.codes), chrom=_chrom(P), **ROH)))))
def _(P, out):
    ind, seg = _api().bed_roh(P.bed, P.dims, chrom=_chrom(P), **ROH)
    return {"ind": ind, "seg": seg}


def _pairs(P):
    rng = P.rng(6)
    a = rng.integers(0, P.n, size=(400, 2))
    a = a[a[:, 0] != a[:, 1]]
    a.sort(axis=1)
    return np.concatenate([[[0, 1], [0, P.n - 1], [P.n - 2, P.n - 1]], a]).astype(np.int32)


def _bed_g_called(P):
    return _r_api().ibd_genotypes_bed(P.codes)


@case("ibd", "runs", ["ibd"], "s203", "b411",
      lambda P, res: _same(res, dict(zip(("pair", "seg"), _r_api().ibd_host(P.Mt8, None, pairs=_pairs(P), chrom=_chrom(P), **IBD)))))
def _(P, out):
    tab, seg = _api().ibd(P.fM, P.dims, pairs=_pairs(P), chrom=_chrom(P), **IBD)
    return {"pair": tab, "seg": seg}


def _truth_bed_ibd(P, res):
    g, called = _bed_g_called(P)
    _same(res, dict(zip(("pair", "seg"), _r_api().ibd_host(g, called, pairs=_pairs(P), chrom=_chrom(P), **IBD))))


@case("bed_ibd", "runs", ["bed_ibd"], "s203", "b411", _truth_bed_ibd)
def _(P, out):
    tab, seg = _api().bed_ibd(P.bed, P.dims, pairs=_pairs(P), chrom=_chrom(P), **IBD)
    return {"pair": tab, "seg": seg}


def _trios(P):
    from test_gpu_mendel import trio_list
    return trio_list(P.n, 70, P.n)


@case("mendel", "runs", ["mendel"], "s203", "b411",
      lambda P, res: _same(res, dict(zip(("trio", "marker"), _r_api().mendel_host(P.Mt8, None, _trios(P))))))
def _(P, out):
    trio, marker = _api().mendel(P.fM, P.dims, _trios(P))
    return {"trio": trio, "marker": marker}


def _truth_bed_mendel(P, res):
    g, called = _bed_g_called(P)
    _same(res, dict(zip(("trio", "marker"), _r_api().mendel_host(g, called, _trios(P)))))


@case("bed_mendel", "runs", ["bed_mendel"], "s203", "b411", _truth_bed_mendel)
def _(P, out):
    trio, marker = _api().bed_mendel(P.bed, P.dims, _trios(P))
    return {"trio": trio, "marker": marker}


def _parent_lists(P):
    return np.arange(0, 40), np.arange(40, 40 + 33), np.arange(100, 100 + 17)


@case("parentage", "runs", ["parentage"], "s203", "b411",
      lambda P, res: _same(res, {"best": _r_api().parentage_host(P.Mt8, None, *_parent_lists(P), min_overlap=5)}))
def _(P, out):
    return {"best": _api().parentage(P.fM, P.dims, *_parent_lists(P), min_overlap=5)}


def _truth_bed_parentage(P, res):
    g, called = _bed_g_called(P)
    _same(res, {"best": _r_api().parentage_host(g, called, *_parent_lists(P), min_overlap=5)})


@case("bed_parentage", "runs", ["bed_parentage"], "s203", "b411", _truth_bed_parentage)
def _(P, out):
    return {"best": _api().bed_parentage(P.bed, P.dims, *_parent_lists(P), min_overlap=5)}


TDT = dict(seed=5, first=1, R=40)


@case("tdt", "runs", ["tdt"], "s203", "b411", lambda P, res: _same(res, _r_api().tdt_host(P.Mt8, None, _trios(P), **TDT)))
def _(P, out):
    return _api().tdt(P.fM, P.dims, _trios(P), **TDT)


def _truth_bed_tdt(P, res):
    g, called = _bed_g_called(P)
    _same(res, _r_api().tdt_host(g, called, _trios(P), **TDT))


@case("bed_tdt", "runs", ["bed_tdt"], "s203", "b411", _truth_bed_tdt)
def _(P, out):
    return _api().bed_tdt(P.bed, P.dims, _trios(P), **TDT)


# ------------------------------------------------------------------------------------------------ Grams and scores
def _q(P):
    q = P.rng(7).integers(0, 1 << 21, size=P.L)
    q[:4] = (0, 1, 127, (1 << 21) - 1)
    return q


def _truth_wgram(P, res):
    from test_grm_host import np_wgram
    _same(res, {"Q": np_wgram(P.Mt8.T, _q(P))})


@case("weighted_gram resident", "grams", ["weighted_gram"], "s203", "b411", _truth_wgram)
def _(P, out):
    return {"Q": _api().weighted_gram(P.fM, P.dims, _q(P))}


@case("weighted_gram windows", "grams", ["weighted_gram"], "s203", "b411", _truth_wgram)
def _(P, out):
    with env(EAGLE_HIP_MAX_RESIDENT_GB="0.001"):       # marker windows of 256: two at L = 389, the last of 133
        return {"Q": _api().weighted_gram(P.fM, P.dims, _q(P))}


def _weights(P, length):
    w = P.rng(8).integers(-(1 << 30), (1 << 30) + 1, size=(3, length))
    w[0, :3] = (1 << 30, -(1 << 30), 0)
    return w


def _truth_scores(by_marker):
    def truth(P, res):
        from scores_truth import np_scores
        G8 = P.Mt8 if by_marker else np.ascontiguousarray(P.Mt8.T)
        _same(res, {"S": np_scores(G8, _weights(P, G8.shape[1]))})
    return truth


@case("sample_scores", "grams", ["sample_scores"], "s203", "b411", _truth_scores(False))
def _(P, out):
    return {"S": _api().sample_scores(P.fM, P.dims, _weights(P, P.L))}


@case("marker_scores", "grams", ["marker_scores"], "s203", "b411", _truth_scores(True))
def _(P, out):
    return {"S": _api().marker_scores(P.fMt, P.dims, _weights(P, P.n))}


# ------------------------------------------------------------------------------------------------ association and structure
def _trait(P):
    return P.rng(9).integers(-1000, 1001, size=P.n).astype(np.int32)


def _truth_epi_pairs(P, res):
    want = _r_api().epistasis_host(P.Mt8.T, _trait(P), None, chrom=_chrom(P), gap=2, min_stat=6.0)
    assert res["nhits"] == want["nhits"] and res["ntested"] == want["ntested"]
    assert tuple(res["max"][:2]) == tuple(want["max"][:2]) and res["max"][2] == want["max"][2]      # (a hit exists: not NaN)
    _same(res, want, keys=("hit_ij", "hit_stat", "hit_mom"))


@case("epistasis_pairs", "assoc", ["epistasis_pairs"], "s203e", "b411e", _truth_epi_pairs)
def _(P, out):
    res = _api().epistasis_pairs(P.fMt, P.dims, _trait(P), chrom=_chrom(P), gap=2, min_stat=6.0)
    res["max"] = np.array(res["max"], dtype=np.float64)
    return res


def _truth_epi_loci(P, res):
    want = _r_api().epistasis_host(P.Mt8.T, _trait(P), _loci(P))
    _same(res, {"stat": want["stat"], "mom": want["mom"]})


@case("epistasis_loci", "assoc", ["epistasis_loci"], "s203e", "b411e", _truth_epi_loci)
def _(P, out):
    stat, mom = _api().epistasis_loci(P.fMt, P.dims, _trait(P), _loci(P))
    return {"stat": stat, "mom": mom}


def _strata(P):
    return (np.arange(P.n) % 3).astype(np.int32)


@case("maxt", "assoc", ["maxt"], "s203", "b411",
      lambda P, res: _same(res, _r_api().maxt_host(P.Mt8, _trait(P), None, _strata(P), 3, 1, 40)))
def _(P, out):
    return _api().maxt(P.fMt, P.dims, _trait(P), strata=_strata(P), seed=3, first=1, R=40)


LOGISTIC_TOL = 1e-10


def _logistic_case(firth):
    def run(P, out):
        x = P.extra
        stat, info = _api().logistic(P.fMt, P.dims, x["st"], x["X"], firth=firth, tol=LOGISTIC_TOL, max_iter=200 if firth else 50)
        return {"stat": stat, "info": info}

    def truth(P, res):
        """The bounds of tests/test_gpu_logistic.py::check_panel: ML on the markers whose fit exists with a clear margin, Firth on the
        panel's firth_rows."""
        import logistic_truth as T
        x, t, stat, info = P.extra, P.extra["t"], res["stat"], res["info"]
        if firth == 0:
            good = (t["ok"] == 1) & (t["maxeta"] <= T.ETA_CLEAR) & (t["cond"] <= 1e6)
            assert good.mean() > 0.95
            bg, rse, rll = T.ml_bounds(P.n, LOGISTIC_TOL, {k: v[good] for k, v in t.items()})
            assert np.all(info[good, 0] == 0)
            assert np.all(np.abs(stat[good, 0] - t["gamma"][good]) <= bg)
            assert np.all(np.abs(stat[good, 1] / t["se"][good] - 1.0) <= rse) and np.all(np.abs(stat[good, 3] / t["ll"][good] - 1.0) <= rll)
        else:
            rows = [m for m in x["firth_rows"] if t["f_ok"][m] == 1 and t["f_cond"][m] <= 1e6]
            assert len(rows) >= len(x["firth_rows"]) - 1 and np.all(info[:, 0] >= 256)
            for m in rows:
                fg, fse = T.firth_bounds(P.n, LOGISTIC_TOL, t, m)
                assert info[m, 0] == 256, (m, info[m])
                assert abs(stat[m, 0] - t["f_gamma"][m]) <= fg and abs(stat[m, 1] - t["f_se"][m]) <= fse * t["f_se"][m], m
    return run, truth


for _f, _n in ((0, "ML"), (1, "Firth")):
    _run, _truth = _logistic_case(_f)
    case("logistic " + _n, "assoc", ["logistic"], "log257", "log1003", _truth)(_run)


def _truth_admix(P, res):
    import admixture_truth as T
    K = 3
    Q, F = T.planted_inputs(P.n, P.L, K, P.n + K)
    want = _r_api().admixture_host(P.Mt8, Q, F, 1)
    T.assert_close((res["Q"], res["F"], res["ll"][0], res["ll"][1]), (want[0], want[1], want[2][0], want[2][1]), P.n, P.L, K, "device")
    assert np.max(np.abs(res["Q"].sum(axis=1) - 1.0)) <= (2 * K - 1) * 2.0 ** -53


@case("admixture_em", "assoc", ["admixture_em"], "s203", "b411", _truth_admix)
def _(P, out):
    import admixture_truth as T
    Q, F = T.planted_inputs(P.n, P.L, 3, P.n + 3)
    Qo, Fo, ll = _api().admixture_em(P.fMt, P.dims, Q, F, 1)
    return {"Q": Qo, "F": Fo, "ll": ll}


# ------------------------------------------------------------------------------------------------ model algebra
class Shape:
    """The `panel` of a case without genotypes: its size alone."""
    def __init__(self, n):
        self.n, self.tag = n, "n%d" % n

    def rng(self, salt):
        return np.random.default_rng(self.n + salt)


PANELS["n150"] = lambda: Shape(150)
PANELS["n301"] = lambda: Shape(301)


def _spd(P):
    B = P.rng(10).standard_normal((P.n, P.n + 3))
    return B @ B.T / P.n + 0.5 * np.eye(P.n)


def _truth_eig(P, res):
    A = _spd(P)
    w_ref = np.linalg.eigvalsh(A)[::-1]                # the bounds of tests/test_linalg_abi.py
    np.testing.assert_allclose(res["w"], w_ref, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(A @ res["U"], res["U"] * res["w"], rtol=0, atol=1e-10 * res["w"][0])
    np.testing.assert_allclose(res["U"].T @ res["U"], np.eye(P.n), atol=1e-11)
    np.testing.assert_allclose(res["w_only"], w_ref, rtol=1e-11, atol=1e-13)


@case("sym_eig", "linalg", ["sym_eig"], "n150", "n301", _truth_eig)
def _(P, out):
    api = _api()
    w, U = api.sym_eig(_spd(P))
    return {"w": w, "U": U, "w_only": api.sym_eig(_spd(P), only_values=True)[0]}


def _truth_chol2inv(P, res):
    np.testing.assert_allclose(res["Ai"], np.linalg.inv(_spd(P)), rtol=1e-9, atol=1e-11)
    assert np.array_equal(res["Ai"], res["Ai"].T)


@case("chol2inv", "linalg", ["chol2inv"], "n150", "n301", _truth_chol2inv)
def _(P, out):
    return {"Ai": _api().chol2inv(_spd(P))}


def _general(P):
    return P.rng(11).standard_normal((P.n, P.n)) + P.n * np.eye(P.n)


@case("inverse", "linalg", ["inverse"], "n150", "n301",
      lambda P, res: np.testing.assert_allclose(res["Gi"], np.linalg.inv(_general(P)), rtol=1e-9, atol=1e-12))
def _(P, out):
    return {"Gi": _api().inverse(_general(P))}


def _matmul_operands(P):
    rng = P.rng(12)
    m, k, n = 4 * P.n + 100, P.n - 20, P.n + 107     # 700 x 130 x 257 at n = 150
    return (rng.standard_normal((m, k)), rng.standard_normal((k, n)), rng.integers(-9, 10, size=(m, k)).astype(np.float64),
            rng.integers(-9, 10, size=(k, n)).astype(np.float64))


def _truth_matmul(P, res):
    A, B, Ai, Bi = _matmul_operands(P)
    np.testing.assert_allclose(res["AB"], A @ B, rtol=0, atol=1e-12 * A.shape[1])
    np.testing.assert_array_equal(res["ABi"], Ai @ Bi)                     # integer-valued: exact in fp64
    np.testing.assert_array_equal(res["ABf"], Ai @ Bi)


@case("matmul", "linalg", ["matmul"], "n150", "n301", _truth_matmul)
def _(P, out):
    api = _api()
    A, B, Ai, Bi = _matmul_operands(P)
    return {"AB": api.matmul(A, B), "ABi": api.matmul(Ai, Bi), "ABf": api.matmul(np.asfortranarray(Ai), np.asfortranarray(Bi))}


def _truth_sqrt(P, res):
    MMt = _spd(P)
    np.testing.assert_allclose(res["sq"] @ res["sq"], MMt, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["sq"] @ res["inv"], np.eye(P.n), atol=1e-11)
    assert np.array_equal(res["sq"], res["sq"].T) and np.array_equal(res["inv"], res["inv"].T)
    assert abs(res["tr"] - P.n) < 1e-9
    w, U = np.linalg.eigh(MMt)
    np.testing.assert_allclose(res["sq"], (U * np.sqrt(w)) @ U.T, rtol=0, atol=1e-12)


@case("mmt_sqrt_and_sqrtinv", "linalg", ["mmt_sqrt_and_sqrtinv"], "n150", "n301", _truth_sqrt)
def _(P, out):
    sq, inv, tr = _api().mmt_sqrt_and_sqrtinv(_spd(P))
    return {"sq": sq, "inv": inv, "tr": tr}


# ------------------------------------------------------------------------------------------------ end to end
QTL = 700


def _e2e_trait(P):
    rng = np.random.default_rng(3)                      # the trait of tests/test_gpu_lmm.py::test_gwas_end_to_end
    X = np.column_stack([np.ones(P.n), rng.standard_normal(P.n)])
    y = X @ [1.0, 0.3] + 1.5 * P.Mt8[QTL].astype(np.float64) + 0.06 * (P.Mt8.astype(np.float64).T @ rng.standard_normal(P.L)) \
        + 1.5 * rng.standard_normal(P.n)
    return X, y


def _truth_e2e(P, res):
    assert QTL + 1 in res["all_picks"].tolist()
    ok = res["gwas_code"] == 0
    assert ok.mean() > 0.9 and set(res["gwas_code"].tolist()) <= {0, 3, 4}
    assert int(np.argmin(res["gwas_p"])) == QTL and int(np.argmax(res["gwas_score"])) == QTL


@case("am.AM and am.GWAS", "e2e", [], "e2e", "e2eb", _truth_e2e)
def _(P, out):
    from eagleeverything_amd import am
    X, y = _e2e_trait(P)
    be = am.SpectralBackend()
    res = am.AM(y, X, P.geno, maxit=3, backend=be)
    gw = am.GWAS(y, X, P.geno, backend=be)              # on the resident Z of AM()
    o = {"selected_loci": np.asarray(res["selected_loci"], dtype=np.int64), "all_picks": np.asarray(res["all_picks"], dtype=np.int64),
         "extBIC": np.asarray(res["extBIC"], dtype=np.float64), "ve": float(res["ve"]), "vg": float(res["vg"])}
    for k in am._GWAS_EXACT + ("code", "iterations", "score", "p_score", "p"):
        o["gwas_" + k] = np.asarray(gw[k])
    return o


# ------------------------------------------------------------------------------------------------ the test
def _counters(api):
    return np.array(list(api.scan_operand_cache_stats()) + list(api.w8_keep_stats()) + list(api.view_load_counts().values()), dtype=np.int64)


def _canon(v):
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, v.tobytes())
    if isinstance(v, float):
        return np.float64(v).tobytes()
    return v


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    global ROOT_DIR
    api = _api()
    assert api.device_info()["arch"].startswith("gfx950")
    ROOT_DIR = str(tmp_path_factory.mktemp("poison"))
    yield ROOT_DIR
    os.environ.pop(HOOK, None)
    api.close_all()


def _step(c, fill, root, tag):
    """One step of a case on a context of its own: hook unset (fill None) or set, the larger call first under the hook."""
    api = _api()
    api.close_all()
    if fill is None:
        os.environ.pop(HOOK, None)
    else:
        os.environ[HOOK] = str(fill)
    try:
        api.context()                                   # the context itself is opened under the hook
        outs = []
        for which, key in (("big", c.big), ("small", c.small)):
            if which == "big" and fill is None:
                continue
            out = os.path.join(root, "%s_%s_%s" % (c.name.replace(" ", "_").replace(".", "_"), tag, which))
            os.makedirs(out)
            before = _counters(api)
            res = dict(c.run(panel(key), out))
            res["counters"] = _counters(api) - before
            shutil.rmtree(out)
            outs.append(res)
        return outs[-1]
    finally:
        os.environ.pop(HOOK, None)
        api.close_all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES), ids=["%s-%s" % (c.family, c.name.replace(" ", "_")) for c in CASES.values()])
def test_poisoned(name, workdir):
    c = CASES[name]
    clean = _step(c, None, workdir, "clean")
    for fill in FILLS:
        dirty = _step(c, fill, workdir, "%02x" % fill)
        assert sorted(dirty) == sorted(clean)
        bad = [k for k in clean if _canon(dirty[k]) != _canon(clean[k])]
        assert not bad, "fill 0x%02X: %s differ from the run on clean memory" % (fill, bad)
        if c.truth is not None:
            c.truth(panel(c.small), dirty)


# ---- kept state: what a context keeps between calls is not scratch, the hook must leave it alone ----
def _keeper_cached_s(P, api):
    api.set_scan_mode(1)
    S, V, ahat = _scan_operands(P)
    call = lambda: api.calculate_a_and_vara_rcpp(P.fMt, NA, S, V, 8.0, (P.L, P.n), ahat)
    return call, lambda: api.scan_operand_cache_stats()[0]


def _keeper_w8_digits(P, api):
    api.set_scan_mode(1)
    api.set_w_mode(2)
    S, V, ahat = _scan_operands(P)
    call = lambda: api.calculate_a_and_vara_rcpp(P.fMt, NA, S, V, 8.0, (P.L, P.n), ahat)
    return call, lambda: api.w8_keep_stats()[0]


def _keeper_resident_z(P, api):
    import exact_spectral as xs
    c = P.extra["case"]
    api.spectral_prepare(P.fMt, (c["L"], c["n"]), c["U"], 8.0)
    op = xs.single_op(c, xs.single_ps(c)[-1])
    call = lambda: api.spectral_scan(c["lam"], op["X"].astype(np.float64), op["y"].astype(np.float64), op["varE"], op["varG"], c["L"])
    # (the library counts nothing here: a scan has no other Z to run on than the one the prepare left, so the hit is that both scans, with
    # no prepare between them, return the bytes of the run on clean memory -- asserted below -- while the record of the prepare still stands)
    return call, lambda: int(api.spectral_holds(P.fMt, c["U"]))


def _keeper_resident_image(P, api):
    nd = api.ReshapeM_rcpp(P.fM, P.fMt, [3, P.n - 1, 77], P.dims, view=True)
    api.marker_counts(P.fMt, P.dims)                                       # the source's image becomes resident
    # ReadBlock keeps no image of its own: every call loads its rows of the alias anew, through the keep-map, from the source's image
    call = lambda: {"head": api.ReadBlock(P.fMt + "tmp", 0, nd[0], 7), "tail": api.ReadBlock(P.fMt + "tmp", P.L - 5, nd[0], 5)}

    def hits():                                                            # windows of the alias served from the resident source image,
        c = api.view_load_counts()                                         # and none from the sidecar, the text or the line scanner
        return c["resident"] if c["sidecar"] + c["text"] + c["scanner"] == 0 else -1
    return call, hits


KEEPERS = {"cached S": ("s257", _keeper_cached_s, 1), "W8 digits": ("s257", _keeper_w8_digits, 1), "resident Z": ("xs257", _keeper_resident_z, 0),
           "resident genotype image": ("s203", _keeper_resident_image, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("what", list(KEEPERS))
def test_kept_state_survives(what, workdir):
    key, make, gain = KEEPERS[what]
    api = _api()
    P = panel(key)
    results = {}
    for fill in (None, 0xFF):
        api.close_all()
        os.environ.pop(HOOK, None)
        if fill is not None:
            os.environ[HOOK] = str(fill)
        try:
            api.context()
            call, hits = make(P, api)
            first = call()
            h0 = hits()
            second = call()
            assert hits() - h0 >= gain and hits() >= 1, "%s: the second call did not find what the first left" % what
            results[fill] = [{k: _canon(np.asarray(v)) for k, v in r.items()} for r in (first, second)]
        finally:
            os.environ.pop(HOOK, None)
            api.close_all()
    assert results[None][0] == results[None][1], "a second call on clean memory gives other bytes"
    assert results[0xFF][0] == results[None][0] and results[0xFF][1] == results[None][0]


# ---- the instrument itself: the bytes are really there ----
@pytest.mark.gpu
def test_hook_fills_allocations_and_handouts(workdir):
    """The context's scratch page is filled where it is allocated; the context's fp4 buffer where it is allocated and, handed out again,
    in the part handed out and no further; with the hook unset again nothing is touched."""
    import ctypes as C
    from eagleeverything_amd import _lib
    api, L, hip = _api(), _lib.load(), C.CDLL("libamdhip64.so")
    scratch, f4 = L.eagle_ctx_scratch, L.eagle_ctx_f4_buffer            # (csrc/eagle_internal.h; not part of the public ABI)
    scratch.restype, scratch.argtypes = C.c_void_p, [C.c_void_p]
    f4.restype, f4.argtypes = C.c_void_p, [C.c_void_p, C.c_size_t]

    def peek(ptr, nbytes):
        buf = (C.c_ubyte * nbytes)()
        assert hip.hipMemcpy(buf, C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0      # hipMemcpyDeviceToHost
        return bytes(buf)

    api.close_all()
    try:
        os.environ[HOOK] = str(0x55)
        ctx = api.context()
        assert peek(scratch(ctx), 8192) == b"\x55" * 8192
        p = f4(ctx, 4096)
        assert p and peek(p, 4096) == b"\x55" * 4096
        os.environ[HOOK] = str(0x7F)
        assert f4(ctx, 1000) == p and peek(p, 4096) == b"\x7f" * 1000 + b"\x55" * 3096
        os.environ[HOOK] = "256"                                         # not a byte: the hook is off
        assert f4(ctx, 4096) == p and peek(p, 4096) == b"\x7f" * 1000 + b"\x55" * 3096
        os.environ.pop(HOOK)
        assert f4(ctx, 2000) == p and peek(p, 4096) == b"\x7f" * 1000 + b"\x55" * 3096
    finally:
        os.environ.pop(HOOK, None)
        api.close_all()
