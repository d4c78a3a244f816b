"""Truth for the logistic fits of include/eagle_hip.h section 1b''''iv, in mpmath at 40 digits: the root of U(beta) = 0 (maximum
likelihood) by Newton's iteration and the root of U*(beta) = 0 (Firth) by the iteration beta += I^-1 U*, both from beta = 0 and both
written here from the model alone -- nothing is shared with r_api.logistic_host or the kernel but the model -- then I^-1, se and the
log-likelihood at the root and the two numbers the error bounds need: cond(I) and sum_k |I^-1_jk| sum_i |x~_ik|.

The panels of tests/test_gpu_logistic.py are defined here (panel()).  Their truth costs minutes of mpmath, so it is computed once
(`python tests/logistic_truth.py` rewrites tests/golden/logistic_truth.npz) and the file is keyed by a digest of each panel's
inputs: golden() refuses a file that was made from other inputs, and tests/test_logistic_host.py recomputes entries of it live."""
import hashlib
import os

import mpmath
import numpy as np

DPS = 40
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logistic_truth.npz")
ETA_CLEAR = 30.0           # the device calls separation at max |eta| > 40: below 30 at the root the margin is clear
NS = [20, 63, 64, 65, 67, 255, 257, 1003]
LS = [1, 3, 4, 5, 129]
CS = [1, 2, 4, 15]
FIELDS = ("ok", "gamma", "se", "ll", "cond", "round_g", "round_all", "rowabs", "maxeta")
FIRTH_FIELDS = ("f_ok", "f_gamma", "f_se", "f_ratio", "f_cond", "f_round_g", "f_round_all", "f_rowabs")


# ------------------------------------------------------------------------------------------------ the fits
def _design(g012, status, X):
    """The used individuals' rows (x_i, g_i) as mpf columns and y as ints."""
    st = np.asarray(status).astype(np.int64).ravel()
    used = np.flatnonzero(st >= 0)
    Xt = np.column_stack([np.asarray(X, dtype=np.float64)[used], np.asarray(g012, dtype=np.float64)[used]])
    cols = [[mpmath.mpf(float(v)) for v in Xt[:, j]] for j in range(Xt.shape[1])]
    return Xt, cols, [int(v) for v in st[used]]


def _evaluate(cols, y, beta, want_I=True):
    n, p = len(y), len(cols)
    eta = [mpmath.fsum(cols[j][i] * beta[j] for j in range(p)) for i in range(n)]
    mu = [1 / (1 + mpmath.exp(-e)) for e in eta]
    w = [m * (1 - m) for m in mu]
    res = [y[i] - mu[i] for i in range(n)]
    U = [mpmath.fdot(res, cols[j]) for j in range(p)]
    ll = mpmath.fsum(y[i] * eta[i] - mpmath.log(1 + mpmath.exp(eta[i])) for i in range(n))
    I = None
    if want_I:
        I = mpmath.zeros(p)
        for j in range(p):
            wj = [w[i] * cols[j][i] for i in range(n)]
            for k in range(j + 1):
                I[j, k] = I[k, j] = mpmath.fdot(wj, cols[k])
    return eta, mu, w, U, I, ll


def _step(I, U):
    try:
        d = mpmath.lu_solve(I, mpmath.matrix(U))
    except ZeroDivisionError:
        return None
    d = [d[j] for j in range(len(U))]
    md = max(abs(v) for v in d)
    if md > 5:
        d = [v * 5 / md for v in d]
    return d, md


def ml_root(cols, y, max_iter=80):
    """(beta, max |eta| at the root) or None: separated, singular or not there after max_iter steps."""
    p = len(cols)
    beta = [mpmath.mpf(0)] * p
    for _ in range(max_iter):
        eta, _, _, U, I, _ = _evaluate(cols, y, beta)
        if max(abs(e) for e in eta) > 200:
            return None
        s = _step(I, U)
        if s is None:
            return None
        beta = [b + d for b, d in zip(beta, s[0])]
        if s[1] < mpmath.mpf(10) ** -34:
            return beta, float(max(abs(e) for e in eta))
    return None


def firth_root(cols, y, max_iter=400):
    """(beta, ratio of the last two steps' sizes) or None.  The iteration converges linearly: the ratio is its contraction."""
    n, p = len(y), len(cols)
    beta = [mpmath.mpf(0)] * p
    steps = []
    for _ in range(max_iter):
        _, mu, w, _, I, _ = _evaluate(cols, y, beta)
        try:
            Inv = I ** -1
        except ZeroDivisionError:
            return None
        h = []
        for i in range(n):
            r = [cols[j][i] for j in range(p)]
            t = [mpmath.fdot([Inv[j, k] for k in range(p)], r) for j in range(p)]
            h.append(w[i] * mpmath.fdot(r, t))
        res = [y[i] - mu[i] + h[i] * (mpmath.mpf(1) / 2 - mu[i]) for i in range(n)]
        Us = [mpmath.fdot(res, cols[j]) for j in range(p)]
        s = _step(I, Us)
        if s is None:
            return None
        beta = [b + d for b, d in zip(beta, s[0])]
        steps.append(s[1])
        if s[1] < mpmath.mpf(10) ** -30:
            return beta, float(steps[-1] / steps[-2]) if len(steps) > 1 and steps[-2] > 0 else 0.0
    return None


def _at_root(Xt, cols, y, beta):
    """se, log-likelihood, cond(I) and the sensitivities at beta (gamma is the last parameter)."""
    p = len(cols)
    eta, _, _, _, I, ll = _evaluate(cols, y, beta)
    Inv = I ** -1
    colabs = np.abs(Xt).sum(axis=0)
    rnd = [float(mpmath.fsum(abs(Inv[j, k]) * colabs[k] for k in range(p))) for j in range(p)]
    If = np.array([[float(I[j, k]) for k in range(p)] for j in range(p)])
    return {"gamma": float(beta[-1]), "se": float(mpmath.sqrt(Inv[p - 1, p - 1])), "ll": float(ll), "cond": float(np.linalg.cond(If)),
            "round_g": rnd[-1], "round_all": max(rnd), "rowabs": float(np.abs(Xt).sum(axis=1).max()),
            "maxeta": float(max(abs(e) for e in eta))}


def marker_truth(g012, status, X, firth=False):
    """One marker: the ML truth (FIELDS) and with firth=True the Firth truth too (FIRTH_FIELDS).  ok = 0 where no ML fit exists."""
    with mpmath.workdps(DPS):
        Xt, cols, y = _design(g012, status, X)
        out = dict.fromkeys(FIELDS + FIRTH_FIELDS, float("nan"))
        out["ok"] = out["f_ok"] = 0.0
        if np.ptp(Xt[:, -1]) == 0:                                       # monomorphic among the used individuals
            return out
        r = ml_root(cols, y)
        if r is not None:
            out.update(_at_root(Xt, cols, y, r[0]))
            out["ok"] = 1.0
        if firth:
            f = firth_root(cols, y)
            if f is not None:
                a = _at_root(Xt, cols, y, f[0])
                out.update(f_ok=1.0, f_gamma=a["gamma"], f_se=a["se"], f_ratio=f[1], f_cond=a["cond"], f_round_g=a["round_g"], f_round_all=a["round_all"],
                           f_rowabs=a["rowabs"])
        return out


U53 = 2.0 ** -53


def ml_bounds(n, tol, t, m=None):
    """(bound of |gamma - gamma*|, relative bound of se, relative bound of the log-likelihood) of a converged ML fit with stop rule
    `tol` over n individuals, from the truth t (row m of a panel's truth).  gamma: the stop rule -- Newton converges quadratically, the
    error left after a step <= tol is far below tol -- plus the sensitivity of the root to the rounding of U, 8 (n + 16) u sum_k
    |I^-1_gk| sum_i |x~_ik|.  se and the log-likelihood are those of the last evaluation, whose point is within tol of the reported
    beta, which is within `all` = tol + the largest such sensitivity of the root: eta moves by at most rowabs (tol + all) = eps, w by
    the factor e^eps at most (|d log w / d eta| <= 1), so I lies between e^-eps I and e^eps I and se moves by eps relative at most;
    every term of the log-likelihood moves by at most eps (|y - mu| <= 1).  Their own rounding is 8 (n + 16) u cond(I)."""
    g = (lambda k: t[k]) if m is None else (lambda k: t[k][m])
    rt = 8.0 * (n + 16) * U53
    ball = tol + rt * g("round_all")
    eps = g("rowabs") * (tol + ball)
    return tol + rt * g("round_g"), rt * g("cond") + eps, rt * g("cond") + n * eps / abs(g("ll"))


def firth_bounds(n, tol, t, m=None):
    """(bound of |gamma - gamma*|, relative bound of se) of a converged Firth fit: the iteration converges linearly, so a step <= tol
    leaves tol r / (1 - r) <= 9 tol at a contraction r <= 0.9 (f_ratio, which the caller asserts); the bound is 16 tol plus the rounding
    term of ml_bounds at the Firth root."""
    g = (lambda k: t[k]) if m is None else (lambda k: t[k][m])
    rt = 8.0 * (n + 16) * U53
    ball = 16.0 * tol + rt * g("f_round_all")
    return 16.0 * tol + rt * g("f_round_g"), rt * g("f_cond") + g("f_rowabs") * (tol + ball)


def score_bounds(Mt8, status, X, beta0, score):
    """Per marker, how far two fp64 evaluations of score = U_g^2 (I^-1)_gg at (beta0, 0) may lie apart: each forms U_g with an error of
    at most dU = 8 (n + 16) u sum_i |g_i| (|y - mu| <= 1) and (I^-1)_gg = v to 8 (n + 16) u cond(I) relative, so the two differ by at
    most 2 [v (2 |U_g| dU + dU^2) + 8 (n + 16) u cond(I) score].  The ingredients (v, cond) are numpy's: a bound needs one digit."""
    st = np.asarray(status)
    used = st >= 0
    n = st.size
    Xu = np.asarray(X, dtype=np.float64)[used]
    mu = 1.0 / (1.0 + np.exp(-(Xu @ np.asarray(beta0, dtype=np.float64))))
    w = mu * (1.0 - mu)
    rt = 8.0 * (n + 16) * U53
    out = np.full(Mt8.shape[0], np.nan)
    for m in range(Mt8.shape[0]):
        g = Mt8[m, used].astype(np.float64) + 1.0
        if np.ptp(g) == 0:
            continue
        Xt = np.column_stack([Xu, g])
        I = Xt.T @ (w[:, None] * Xt)
        v = np.linalg.inv(I)[-1, -1]
        dU = rt * np.abs(g).sum()
        out[m] = 2.0 * (v * (2.0 * np.sqrt(score[m] / v) * dU + dU * dU) + rt * np.linalg.cond(I) * score[m])
    return out


def _one(args):
    return marker_truth(*args)


def panel_truth(Mt8, status, X, firth_rows=(), procs=1):
    """Every marker of a panel -> {field: fp64 (L)}; the Firth truth for the rows in firth_rows."""
    jobs = [(Mt8[m].astype(np.int64) + 1, status, X, m in set(firth_rows)) for m in range(Mt8.shape[0])]
    if procs > 1:
        import multiprocessing
        with multiprocessing.Pool(procs) as pool:
            rows = pool.map(_one, jobs, chunksize=1)
    else:
        rows = [_one(j) for j in jobs]
    return {k: np.array([r[k] for r in rows], dtype=np.float64) for k in FIELDS + FIRTH_FIELDS}


# ------------------------------------------------------------------------------------------------ the panels
def covariates(n, c, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])


def draw_status(X, seed, extra=None):
    """Status from a logistic model on the covariates (plus `extra` on the logit scale), a tenth of the individuals not used (-1), and
    an unused individual on either side of every multiple of 64."""
    n, c = X.shape
    rng = np.random.default_rng(seed)
    coef = np.concatenate([[-0.2], 0.8 / np.sqrt(max(c - 1, 1)) * np.where(np.arange(c - 1) % 2 == 0, 1.0, -1.0)])
    eta = X @ coef + (0.0 if extra is None else extra)
    st = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.int32)
    st[rng.random(n) < 0.1] = -1
    for b in range(64, n, 64):
        st[b - 1] = st[b] = -1
    if n > 64 and n % 64 == 0:
        st[n - 1] = -1
    return st


def planted(n, L, seed, status):
    """synth genotypes (below 32 individuals the first L markers of 4 L with a minor-allele count of at least 8) with, from L >= 8 on, the last three rows all -1 / 0 / +1 (monomorphic) and row L - 4 separated: its
    carriers (one copy) are exactly the cases."""
    from eagleeverything_amd import synth
    Mt8 = synth.genotypes_marker_major(n, L if n >= 32 else 4 * L, seed=seed)
    if n < 32:                                                           # so few individuals: a minor-allele count filter, as QC would
        mac = np.minimum((Mt8 + 1).sum(axis=1), (1 - Mt8).sum(axis=1))
        Mt8 = np.ascontiguousarray(Mt8[mac >= 8][:L])
        assert Mt8.shape[0] == L
    if L >= 8:
        for r, v in enumerate((-1, 0, 1)):
            Mt8[L - 1 - r] = v
        Mt8[L - 4] = np.where(status == 1, 0, -1)
    return Mt8


def panel(name):
    """(Mt8 (L, n) int8, status (n) int32, X (n, c) fp64, rows with a Firth truth) of a named panel: "n<n>" (L = 300; c = 4, at n = 20
    c = 2), "L<L>" (n = 203, c = 2), "c<c>" (n = 203, L = 100)."""
    kind, v = name[0], int(name[1:])
    n, L, c = {"n": (v, 300, 2 if v == 20 else 4), "L": (203, v, 2), "c": (203, 100, v)}[kind]
    seed = {"n": 1000, "L": 2000, "c": 3000}[kind] + v
    X = covariates(n, c, seed)
    st = draw_status(X, seed + 1)
    Mt8 = planted(n, L, seed + 2, st)
    firth_rows = ()
    if name in ("n67", "n257", "c1", "c15"):
        firth_rows = tuple(range(12)) + (L - 4,)
    return Mt8, st, X, firth_rows


def all_panels():
    return ["n%d" % v for v in NS] + ["L%d" % v for v in LS] + ["c%d" % v for v in CS]


def digest(Mt8, status, X):
    h = hashlib.sha256()
    for a in (np.ascontiguousarray(Mt8, dtype=np.int8), np.ascontiguousarray(status, dtype=np.int32), np.ascontiguousarray(X, dtype=np.float64)):
        h.update(repr(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


_cache = {}


def golden(name):
    """(Mt8, status, X, firth_rows, truth) of a named panel, the truth from tests/golden/logistic_truth.npz after its digest is checked."""
    if "npz" not in _cache:
        _cache["npz"] = dict(np.load(GOLDEN))
    z = _cache["npz"]
    Mt8, st, X, fr = panel(name)
    assert str(z[name + "/digest"]) == digest(Mt8, st, X), "tests/golden/logistic_truth.npz was made from other inputs: " + name
    return Mt8, st, X, fr, {k: z[name + "/" + k] for k in FIELDS + FIRTH_FIELDS}


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {}
    for name in all_panels():
        Mt8, st, X, fr = panel(name)
        t = panel_truth(Mt8, st, X, fr, procs=int(os.environ.get("TRUTH_PROCS", "8")))
        out[name + "/digest"] = np.array(digest(Mt8, st, X))
        for k, v in t.items():
            out[name + "/" + k] = v
        print(name, "ok %d of %d, cond <= 1e6: %d, Firth ok %d" % (t["ok"].sum(), len(t["ok"]), (t["cond"] <= 1e6).sum(), t["f_ok"].sum()), flush=True)
    np.savez_compressed(GOLDEN, **out)
