"""Non-R driver of the AM() forward-selection loop -- host side, numpy/LAPACK.

This is the reference's model loop restated so that "the same SNPs are selected" can be demonstrated end to end on
a box without R: constructX -> calcMMt (GPU) -> emma.REMLE -> extBIC via emma.MLE -> find_qtl (GPU scan + arg-max).
Everything n x n stays on the host by design (north_star keeps emma_REMLE / calculateP / calculateH on host LAPACK);
the two marker-dimension operations go through a `backend` whose default is the HIP library (r_api).

Reference lines (E/ = MyPackage/Eagle/):
  AM loop ........................ E/R/AM.R:400-475 (stop rule :448, maxit :463)
  .calcVC ........................ E/R/calcVC.R:1-8           emma.REMLE  E/R/emma_REMLE.R:27-131
  .calc_extBIC ................... E/R/calc_extBIC.R:1-12     emma.MLE    E/R/emma_MLE.R:2-117
  emma.eigen.R.wo.Z / L.wo.Z ..... E/R/emma_eigen_R_wo_Z.R:2-21, E/R/emma_eigen_L_wo_Z.R:1-12
  constructX / extract_geno ...... E/R/constructX.R:1-24, E/R/extract_geno.R:1-19

With a Z matrix (AM(Zmat=), repeated measures) the variance components and extBIC restate the reference's emma_*_w_Z path in a
reduced t x t form; its own .find_qtl takes no Z and fails (SURVEY.md section 8a, config 5 note), so the scan of that model is this
project's definition.
parity unpinned: the reference records no outputs, and R's uniroot (Brent, tol = eps^0.25) is restated from the
published zeroin algorithm, not from R's source.
"""
import math

import numpy as np
from scipy.special import chdtr, gammaln

from . import host_model

_EPS25 = np.finfo(np.float64).eps ** 0.25  # uniroot's default tol


def _zeroin(f, a, b, tol=_EPS25, maxit=1000):
    """Brent's zeroin (Forsythe, Malcolm & Moler), the algorithm behind R's uniroot."""
    fa, fb = f(a), f(b)
    c, fc = a, fa
    eps = np.finfo(np.float64).eps
    if fa == 0.0:
        return a
    if fb == 0.0:
        return b
    for _ in range(maxit + 1):
        prev_step = b - a
        if abs(fc) < abs(fb):
            a, b, c = b, c, b
            fa, fb, fc = fb, fc, fb
        tol_act = 2 * eps * abs(b) + tol / 2
        new_step = (c - b) / 2
        if abs(new_step) <= tol_act or fb == 0.0:
            return b
        if abs(prev_step) >= tol_act and abs(fa) > abs(fb):
            cb = c - b
            if a == c:
                t1 = fb / fa
                p = cb * t1
                q = 1.0 - t1
            else:
                q = fa / fc
                t1 = fb / fc
                t2 = fb / fa
                p = t2 * (cb * q * (q - t1) - (b - a) * (t1 - 1.0))
                q = (q - 1.0) * (t1 - 1.0) * (t2 - 1.0)
            if p > 0:
                q = -q
            else:
                p = -p
            if p < (0.75 * cb * q - abs(tol_act * q) / 2) and p < abs(prev_step * q / 2):
                new_step = p / q
        if abs(new_step) < tol_act:
            new_step = tol_act if new_step > 0 else -tol_act
        a, fa = b, fb
        b += new_step
        fb = f(b)
        if (fb > 0 and fc > 0) or (fb < 0 and fc < 0):
            c, fc = a, fa
    return b


def emma_eigen_L_wo_Z(K):
    ev, U = host_model.algebra().eigh_desc(K)  # R's eigen(): decreasing order
    return {"values": np.ascontiguousarray(ev), "vectors": U if U.flags.f_contiguous or U.flags.c_contiguous else U.copy()}


def emma_eigen_R_wo_Z(K, X):
    n, q = X.shape
    la = host_model.algebra()
    S = X @ np.linalg.solve(X.T @ X, X.T)      # S = diag(n) - X (X'X)^-1 X', without the n x n identity
    np.negative(S, out=S)
    S.flat[:: n + 1] += 1.0
    K1 = K.copy()                              # K + diag(n)
    K1.flat[:: n + 1] += 1.0
    ev, U = la.eigh_desc(la.mm(la.mm(S, K1), S))
    return {"values": ev[: n - q] - 1.0, "vectors": U[:, : n - q].copy()}


def _grid(ngrids, llim, ulim):
    logdelta = np.arange(ngrids + 1) / ngrids * (ulim - llim) + llim
    return logdelta, np.exp(logdelta)


def _reml_ll(logdelta, lam, etas):
    nq = etas.size
    d = math.exp(logdelta)
    return 0.5 * (nq * (math.log(nq / (2 * math.pi)) - 1 - math.log(np.sum(etas * etas / (lam + d)))) - np.sum(np.log(lam + d)))


def _reml_dll(logdelta, lam, etas):
    nq = etas.size
    d = math.exp(logdelta)
    ld = lam + d
    e2 = etas * etas
    return 0.5 * (nq * np.sum(e2 / (ld * ld)) / np.sum(e2 / ld) - np.sum(1.0 / ld))


def _ml_ll(logdelta, lam, etas, xi):
    n = xi.size
    d = math.exp(logdelta)
    return 0.5 * (n * (math.log(n / (2 * math.pi)) - 1 - math.log(np.sum(etas * etas / (lam + d)))) - np.sum(np.log(xi + d)))


def _ml_dll(logdelta, lam, etas, xi):
    n = xi.size
    d = math.exp(logdelta)
    ld = lam + d
    e2 = etas * etas
    return 0.5 * (n * np.sum(e2 / (ld * ld)) / np.sum(e2 / ld) - np.sum(1.0 / (xi + d)))


def _optimise(dLL, logdelta, llim, ulim, esp, ll_fn, dll_fn):
    """The bracket rule shared by emma.REMLE (:60-76) and emma.MLE (:43-60)."""
    m = logdelta.size
    opt_ld, opt_ll = [], []
    if dLL[0] < esp:
        opt_ld.append(llim); opt_ll.append(ll_fn(llim))
    if dLL[m - 2] > 0 - esp:
        opt_ld.append(ulim); opt_ll.append(ll_fn(ulim))
    for i in range(m - 1):
        if dLL[i] * dLL[i + 1] < 0 - esp * esp and dLL[i] > 0 and dLL[i + 1] < 0:
            r = _zeroin(dll_fn, logdelta[i], logdelta[i + 1])
            opt_ld.append(r); opt_ll.append(ll_fn(r))
    k = int(np.argmax(opt_ll))
    return math.exp(opt_ld[k]), opt_ll[k]


def emma_REMLE(y, X, K, Z=None, ngrids=100, llim=-10, ulim=10, esp=1e-10, eig_R=None, zmodel=None):
    """Z: None, or the repeated-measures design as ind_of_obs (or the dense 0/1 matrix): the reduced form of _emma_z."""
    n, q = y.size, X.shape[1]
    if np.linalg.det(X.T @ X) == 0:
        return {"REML": 0, "delta": 0, "ve": 0, "vg": 0}
    if Z is not None or zmodel is not None:
        r = _emma_z(y, X, K, Z, zmodel, ngrids, llim, ulim, esp, True)
        return {"REML": r[0], "delta": r[1], "ve": r[2] * r[1], "vg": r[2]}
    if eig_R is None:
        eig_R = emma_eigen_R_wo_Z(K, X)
    lam = eig_R["values"]
    etas = eig_R["vectors"].T @ y
    logdelta, delta = _grid(ngrids, llim, ulim)
    Lam = lam[:, None] + delta[None, :]
    E2 = (etas * etas)[:, None]
    dLL = 0.5 * delta * ((n - q) * np.sum(E2 / (Lam * Lam), axis=0) / np.sum(E2 / Lam, axis=0) - np.sum(1.0 / Lam, axis=0))
    maxdelta, maxLL = _optimise(dLL, logdelta, llim, ulim, esp, lambda ld: _reml_ll(ld, lam, etas), lambda ld: _reml_dll(ld, lam, etas))
    maxva = np.sum(etas * etas / (lam + maxdelta)) / (n - q)
    return {"REML": maxLL, "delta": maxdelta, "ve": maxva * maxdelta, "vg": maxva}


def emma_MLE(y, X, K, Z=None, ngrids=100, llim=-10, ulim=10, esp=1e-10, eig_L=None, eig_R=None, zmodel=None):
    n = y.size
    if np.linalg.det(X.T @ X) == 0:
        return {"ML": 0, "delta": 0, "ve": 0, "vg": 0}
    if Z is not None or zmodel is not None:
        r = _emma_z(y, X, K, Z, zmodel, ngrids, llim, ulim, esp, False)
        return {"ML": r[0], "delta": r[1], "ve": r[2] * r[1], "vg": r[2]}
    if eig_L is None:
        eig_L = emma_eigen_L_wo_Z(K)
    if eig_R is None:
        eig_R = emma_eigen_R_wo_Z(K, X)
    lam, xi = eig_R["values"], eig_L["values"]
    etas = eig_R["vectors"].T @ y
    logdelta, delta = _grid(ngrids, llim, ulim)
    Lam = lam[:, None] + delta[None, :]
    Xis = xi[:, None] + delta[None, :]
    E2 = (etas * etas)[:, None]
    dLL = 0.5 * delta * (n * np.sum(E2 / (Lam * Lam), axis=0) / np.sum(E2 / Lam, axis=0) - np.sum(1.0 / Xis, axis=0))
    maxdelta, maxLL = _optimise(dLL, logdelta, llim, ulim, esp, lambda ld: _ml_ll(ld, lam, etas, xi),
                                lambda ld: _ml_dll(ld, lam, etas, xi))
    maxva = np.sum(etas * etas / (lam + maxdelta)) / n
    return {"ML": maxLL, "delta": maxdelta, "ve": maxva * maxdelta, "vg": maxva}


# ---------------------------------------------------------------------------------------------------------------------------
# emma.REMLE / emma.MLE in the eigenbasis of K (K = U diag(lam) U^T, fixed for a whole run), the FaST-LMM identities: with
# Ut = U^T X, ut = U^T y, w_k = 1/(lam_k + delta), A = Ut^T W Ut, b = Ut^T W ut,
#     y^T P y = R = ut^T W ut - b^T A^-1 b,   P y = U r,  r = W (ut - Ut A^-1 b),
#     sum log(eig_R + delta) = sum log(lam + delta) + log det A - log det Ut^T Ut,   tr P = sum w - sum_k w_k^2 (Ut A^-1 Ut^T)_kk,
# so every likelihood evaluation costs O(n q^2) instead of the n^3 eigen() of S (K + I) S (emma_eigen_R_wo_Z).  The functions are
# equal in exact arithmetic to _reml_ll / _reml_dll / _ml_ll / _ml_dll; grid, bracket rule and zeroin are emma_REMLE's / emma_MLE's.
# ---------------------------------------------------------------------------------------------------------------------------
def _eig_fit(lam, Ut, ut, delta):
    """w, Ut^T W Ut, W-weighted residual r and R = y^T P y at one delta (R from the residual: no cancellation)."""
    w = 1.0 / (lam + delta)
    Uw = Ut * w[:, None]
    A = Ut.T @ Uw
    beta = np.linalg.solve(A, Uw.T @ ut)
    e = ut - Ut @ beta
    return w, Uw, A, w * e, float(np.sum(w * e * e))


def _eig_ll(logdelta, lam, Ut, ut, reml, logdet_xtx):
    n, q = Ut.shape
    d = math.exp(logdelta)
    _, _, A, _, R = _eig_fit(lam, Ut, ut, d)
    m = n - q if reml else n
    ll = m * (math.log(m / (2 * math.pi)) - 1 - math.log(R)) - np.sum(np.log(lam + d))
    if reml:
        ll -= np.linalg.slogdet(A)[1] - logdet_xtx
    return 0.5 * ll


def _eig_dll(logdelta, lam, Ut, ut, reml):
    n, q = Ut.shape
    d = math.exp(logdelta)
    w, Uw, A, r, R = _eig_fit(lam, Ut, ut, d)
    trP = np.sum(w)
    if reml:
        trP -= np.sum(np.linalg.inv(A) * (Uw.T @ Uw))   # sum_k w_k^2 (Ut A^-1 Ut^T)_kk = tr(A^-1 Ut^T W^2 Ut)
    return 0.5 * ((n - q if reml else n) * np.sum(r * r) / R - trP)


_grid_memo = []   # [(lam, delta, [W | W^2])]: the same lam and grids serve every trait and iteration of a run


def _grid_weights(lam, delta):
    for lm, dl, WW in _grid_memo:
        if lm is lam and np.array_equal(dl, delta):
            return WW
    Wg = 1.0 / (lam[:, None] + delta[None, :])
    WW = np.hstack([Wg, Wg * Wg])
    _grid_memo[:] = ([e for e in _grid_memo if e[0] is lam] + [(lam, delta, WW)])[-2:]
    return WW


def _eig_grid_dll(lam, Ut, ut, delta, reml):
    """dLL/dlogdelta on the whole grid from one GEMM: the n x (q+1)(q+2)/2 products of [Ut | ut] row entries times the n x 2m
    weights [W | W^2], then (q+1) x (q+1) algebra per grid point."""
    n, q = Ut.shape
    B = np.column_stack([Ut, ut])
    iu, ju = np.triu_indices(q + 1)
    WW = _grid_weights(lam, delta)
    S = (B[:, iu] * B[:, ju]).T @ WW                                 # ((q+1)(q+2)/2) x 2m
    m = delta.size
    M = np.empty((2 * m, q + 1, q + 1))
    M[:, iu, ju] = S.T
    M[:, ju, iu] = S.T
    S1, S2 = M[:m], M[m:]
    A, b = S1[:, :q, :q], S1[:, :q, q]
    beta = np.linalg.solve(A, b[..., None])[..., 0]
    R = S1[:, q, q] - np.einsum("gi,gi->g", b, beta)
    r2 = S2[:, q, q] - 2 * np.einsum("gi,gi->g", beta, S2[:, :q, q]) + np.einsum("gi,gij,gj->g", beta, S2[:, :q, :q], beta)
    trP = WW[:, :m].sum(axis=0)
    if reml:
        trP = trP - np.einsum("gij,gji->g", np.linalg.inv(A), S2[:, :q, :q])
    return 0.5 * delta * ((n - q if reml else n) * r2 / R - trP)


def _emma_eig(lam, UtX, Uty, ngrids, llim, ulim, esp, reml):
    lam = np.asarray(lam, dtype=np.float64).ravel()
    Ut = np.asarray(UtX, dtype=np.float64).reshape(lam.size, -1)
    ut = np.asarray(Uty, dtype=np.float64).ravel()
    n, q = Ut.shape
    xtx = Ut.T @ Ut                                  # = X^T X (U orthogonal)
    if np.linalg.det(xtx) == 0:
        return None
    logdet_xtx = np.linalg.slogdet(xtx)[1]
    logdelta, delta = _grid(ngrids, llim, ulim)
    dLL = _eig_grid_dll(lam, Ut, ut, delta, reml)
    maxdelta, maxLL = _optimise(dLL, logdelta, llim, ulim, esp, lambda ld: _eig_ll(ld, lam, Ut, ut, reml, logdet_xtx),
                                lambda ld: _eig_dll(ld, lam, Ut, ut, reml))
    maxva = _eig_fit(lam, Ut, ut, maxdelta)[4] / (n - q if reml else n)
    return maxLL, maxdelta, maxva


def emma_REMLE_eig(lam, UtX, Uty, ngrids=100, llim=-10, ulim=10, esp=1e-10):
    """emma_REMLE(y, X, K) from lam, U = eigh(K): UtX = U^T X (n x q), Uty = U^T y.  No n^3 work."""
    r = _emma_eig(lam, UtX, Uty, ngrids, llim, ulim, esp, True)
    if r is None:
        return {"REML": 0, "delta": 0, "ve": 0, "vg": 0}
    return {"REML": r[0], "delta": r[1], "ve": r[2] * r[1], "vg": r[2]}


def emma_MLE_eig(lam, UtX, Uty, ngrids=100, llim=-10, ulim=10, esp=1e-10):
    """emma_MLE(y, X, K) from lam, U = eigh(K) (the xi of emma_MLE are lam)."""
    r = _emma_eig(lam, UtX, Uty, ngrids, llim, ulim, esp, False)
    if r is None:
        return {"ML": 0, "delta": 0, "ve": 0, "vg": 0}
    return {"ML": r[0], "delta": r[1], "ve": r[2] * r[1], "vg": r[2]}


# ---------------------------------------------------------------------------------------------------------------------------
# The same for T traits at once (FPR4AM).  Trait t has the design [UtX | last[:, t]] (last = None: UtX
# alone, the null fits of a permutation study) and the trait column UtY[:, t].  The weights [W | W^2] depend on lam only, so the
# 101-point dLL grid of ALL traits is ONE product of the stacked (T (q+1)(q+2)/2) x n column products with them, through
# host_model.algebra().mm (the fp64 GEMM of the device with algebra="device"); bracket rule, zeroin and end-point rule then run
# per trait on the scalar functions of _emma_eig.
# ---------------------------------------------------------------------------------------------------------------------------
def _eig_grid_dll_batch(lam, B, delta, reml):
    """_eig_grid_dll for B = T x n x (q+1), trait t's [Ut_t | ut_t]: T x m values of dLL/dlogdelta from one GEMM."""
    T, n, q1 = B.shape
    q = q1 - 1
    iu, ju = np.triu_indices(q1)
    WW = _grid_weights(lam, delta)
    PT = np.ascontiguousarray((B[:, :, iu] * B[:, :, ju]).transpose(0, 2, 1)).reshape(T * iu.size, n)
    S = np.asarray(host_model.algebra().mm(PT, WW)).reshape(T, iu.size, -1)      # (T (q+1)(q+2)/2) x 2m in one product
    m = delta.size
    M = np.empty((T, 2 * m, q1, q1))
    M[:, :, iu, ju] = S.transpose(0, 2, 1)
    M[:, :, ju, iu] = S.transpose(0, 2, 1)
    S1, S2 = M[:, :m], M[:, m:]
    A, b = S1[..., :q, :q], S1[..., :q, q]
    beta = np.linalg.solve(A, b[..., None])[..., 0]
    R = S1[..., q, q] - np.einsum("tgi,tgi->tg", b, beta)
    r2 = S2[..., q, q] - 2 * np.einsum("tgi,tgi->tg", beta, S2[..., :q, q]) + np.einsum("tgi,tgij,tgj->tg", beta, S2[..., :q, :q], beta)
    trP = WW[:, :m].sum(axis=0)[None, :]
    if reml:
        trP = trP - np.einsum("tgij,tgji->tg", np.linalg.inv(A), S2[..., :q, :q])
    return 0.5 * delta[None, :] * ((n - q if reml else n) * r2 / R - trP)


def _emma_eig_batch(lam, UtX, UtY, last, ngrids, llim, ulim, esp, reml):
    """-> (LL, delta, va), T each; a trait whose X^T X is singular gets 0, 0, 0 (emma_REMLE.R:28-30)."""
    lam = np.asarray(lam, dtype=np.float64).ravel()
    n = lam.size
    Ut0 = np.asarray(UtX, dtype=np.float64).reshape(n, -1)
    UtY = np.asarray(UtY, dtype=np.float64).reshape(n, -1)
    T, q0 = UtY.shape[1], Ut0.shape[1]
    q = q0 if last is None else q0 + 1
    B = np.empty((T, n, q + 1))
    B[:, :, :q0] = Ut0[None]
    if last is not None:
        last = np.asarray(last, dtype=np.float64).reshape(n, -1)
        if last.shape[1] != T:
            raise ValueError("one last column per trait: %d for %d traits" % (last.shape[1], T))
        B[:, :, q0] = last.T
    B[:, :, q] = UtY.T
    LL, dl, va = np.zeros(T), np.zeros(T), np.zeros(T)
    xtx = [Ut0.T @ Ut0] * T if last is None else [B[t, :, :q].T @ B[t, :, :q] for t in range(T)]    # = X_t^T X_t (U orthogonal)
    ok = [t for t in range(T) if np.linalg.det(xtx[t]) != 0]
    if not ok:
        return LL, dl, va
    logdelta, delta = _grid(ngrids, llim, ulim)
    dLL = _eig_grid_dll_batch(lam, B if len(ok) == T else B[ok], delta, reml)
    for k, t in enumerate(ok):
        Ut, ut = np.ascontiguousarray(B[t, :, :q]), np.ascontiguousarray(B[t, :, q])
        logdet_xtx = np.linalg.slogdet(xtx[t])[1]
        dl[t], LL[t] = _optimise(dLL[k], logdelta, llim, ulim, esp, lambda ld: _eig_ll(ld, lam, Ut, ut, reml, logdet_xtx),
                                 lambda ld: _eig_dll(ld, lam, Ut, ut, reml))
        va[t] = _eig_fit(lam, Ut, ut, dl[t])[4] / (n - q if reml else n)
    return LL, dl, va


def emma_REMLE_eig_batch(lam, UtX, UtY, last=None, ngrids=100, llim=-10, ulim=10, esp=1e-10):
    """emma_REMLE_eig for the T columns of UtY (n x T): the design of trait t is UtX (n x q, shared), with last (n x T) given
    [UtX | last[:, t]].  Returns {"REML", "delta", "ve", "vg"} of arrays of length T."""
    LL, dl, va = _emma_eig_batch(lam, UtX, UtY, last, ngrids, llim, ulim, esp, True)
    return {"REML": LL, "delta": dl, "ve": va * dl, "vg": va}


def emma_MLE_eig_batch(lam, UtX, UtY, last=None, ngrids=100, llim=-10, ulim=10, esp=1e-10):
    """emma_MLE_eig for the T columns of UtY; arguments as emma_REMLE_eig_batch.  Returns {"ML", "delta", "ve", "vg"}."""
    LL, dl, va = _emma_eig_batch(lam, UtX, UtY, last, ngrids, llim, ulim, esp, False)
    return {"ML": LL, "delta": dl, "ve": va * dl, "vg": va}


# ---------------------------------------------------------------------------------------------------------------------------
# emma.REMLE / emma.MLE with a Z matrix (emma_REMLE.R:78-128, emma_MLE.R:58-105) in the reduced form of host_model.ZModel: with
# lam, U = eigh(D^1/2 K D^1/2) -- lam are the eigenvalues of the reference's non-symmetric K Z^T Z (emma_eigen_L_w_Z.R:8) --,
# Ut = U^T D^-1/2 Z^T X, ut likewise and Wn the Gram matrix of the rows of [X | y] centred within their individual, H/vg = delta I +
# Z K Z^T has the eigenvalues lam + delta on t directions and delta on the other n - t, so
#     A = X^T (H/vg)^-1 X = Ut^T W Ut + Wn_xx / delta,      R = y^T P y = sum w e^2 + [beta; -1]^T Wn [beta; -1] / delta,
#     log det = sum log(lam + delta) + (n - t) log delta,    tr (H/vg)^-1 = sum w + (n - t) / delta
# -- the etas.2.sq / delta and (n - t) / delta terms of emma_REMLE.R:92-94.  n is the number of records.  Grid, bracket rule, zeroin
# and end-point rule are _optimise, as without Z.  The reference's eigen-route takes only t - q of the t eigenvalues of S Z K Z^T S,
# which is the whole spectrum exactly when every column of X is constant within an individual (X in the column space of Z: the
# intercept, a per-line covariate, a marker column Z m_j); there this equals it, otherwise this is the likelihood of the model and the
# reference's route is not.
# ---------------------------------------------------------------------------------------------------------------------------
def as_ind_of_obs(Z):
    """ind_of_obs (0-based int64) from either form of a Z matrix: the vector itself, or the dense n_obs x t 0/1 matrix."""
    Z = np.asarray(Z)
    if Z.ndim == 2:
        from . import r_api
        return r_api.zmat_index(Z)
    return Z.astype(np.int64).ravel()


def _z_fit(lam, Ut, ut, Wn, delta):
    q = Ut.shape[1]
    w = 1.0 / (lam + delta)
    Uw = Ut * w[:, None]
    A = Ut.T @ Uw + Wn[:q, :q] / delta
    beta = np.linalg.solve(A, Uw.T @ ut + Wn[:q, q] / delta)
    e = ut - Ut @ beta
    c = np.append(beta, -1.0)
    rw = max(float(c @ Wn @ c), 0.0)                  # the within-individual residual sum of squares at beta
    return w, Uw, A, w * e, rw, float(np.sum(w * e * e)) + rw / delta


def _z_ll(logdelta, lam, Ut, ut, Wn, n, reml, logdet_xtx):
    t, q = Ut.shape
    d = math.exp(logdelta)
    _, _, A, _, _, R = _z_fit(lam, Ut, ut, Wn, d)
    m = n - q if reml else n
    ll = m * (math.log(m / (2 * math.pi)) - 1 - math.log(R)) - np.sum(np.log(lam + d)) - (n - t) * logdelta
    if reml:
        ll -= np.linalg.slogdet(A)[1] - logdet_xtx
    return 0.5 * ll


def _z_dll(logdelta, lam, Ut, ut, Wn, n, reml):
    t, q = Ut.shape
    d = math.exp(logdelta)
    w, Uw, A, r, rw, R = _z_fit(lam, Ut, ut, Wn, d)
    trP = np.sum(w) + (n - t) / d
    if reml:
        trP -= np.sum(np.linalg.inv(A) * (Uw.T @ Uw + Wn[:q, :q] / (d * d)))
    return 0.5 * ((n - q if reml else n) * (np.sum(r * r) + rw / (d * d)) / R - trP)


def _emma_z(y, X, K, Z, zmodel, ngrids, llim, ulim, esp, reml):
    if zmodel is None:
        ind = as_ind_of_obs(Z)
        vids = np.bincount(ind, minlength=K.shape[0]) > 0            # complete == FALSE: individuals without a record leave K and Z
        if not vids.all():
            K = K[np.ix_(vids, vids)]
            ind = (np.cumsum(vids) - 1)[ind]
        zmodel = host_model.ZModel(K, ind)
    lam = zmodel.lam
    n = zmodel.n_obs
    if np.size(y) != n or X.shape[0] != n:
        raise ValueError("emma with Z: %d records in Z, %d in y, %d rows of X" % (n, np.size(y), X.shape[0]))
    Ut, ut, Wn = zmodel.reduce(X, y)
    q = Ut.shape[1]
    logdet_xtx = np.linalg.slogdet(Ut.T @ Ut + Wn[:q, :q])[1]        # = log det X^T X
    logdelta, delta = _grid(ngrids, llim, ulim)
    dLL = np.array([dl * _z_dll(ld, lam, Ut, ut, Wn, n, reml) for ld, dl in zip(logdelta, delta)])
    maxdelta, maxLL = _optimise(dLL, logdelta, llim, ulim, esp, lambda ld: _z_ll(ld, lam, Ut, ut, Wn, n, reml, logdet_xtx),
                                lambda ld: _z_dll(ld, lam, Ut, ut, Wn, n, reml))
    maxva = _z_fit(lam, Ut, ut, Wn, maxdelta)[5] / (n - q if reml else n)
    return maxLL, maxdelta, maxva


def calcVC(trait, currentX, MMt, eig_R=None, Z=None, zmodel=None):
    r = emma_REMLE(trait, currentX, MMt, Z=Z, eig_R=eig_R, zmodel=zmodel)
    return {"vg": r["vg"], "ve": r["ve"]}


def _lchoose(n, k):
    return gammaln(n + 1) - gammaln(k + 1) - gammaln(n - k + 1)


def calc_extBIC(trait, currentX, MMt, nmarkers, eig_L=None, eig_R=None, Z=None, zmodel=None, gamma=1.0):
    """calc_extBIC.R:1-12 with the weight gamma on the model-space term; gamma = 1 is the reference's
    value bit for bit, 2 * 1.0 being exact."""
    res = emma_MLE(trait, currentX, MMt, Z=Z, llim=-100, ulim=100, eig_L=eig_L, eig_R=eig_R, zmodel=zmodel)
    BIC = -2 * res["ML"] + (currentX.shape[1] + 1) * math.log(trait.size)
    return BIC + 2 * gamma * _lchoose(nmarkers, currentX.shape[1] - 1)


class HipBackend:
    """The two marker-dimension calls of the loop on the GPU (r_api mirrors the R wrappers' marshalling)."""

    def __init__(self, device=0):
        from . import r_api, rcpp_api
        self.r_api, self.rcpp_api, self.device = r_api, rcpp_api, device

    def calcMMt(self, geno, availmemGb, ncpu, selected_loci, quiet):
        return self.r_api.calcMMt(geno, availmemGb, ncpu, selected_loci, quiet, device=self.device)

    def find_qtl(self, **kw):
        return self.r_api.find_qtl(device=self.device, **kw)

    def extract_geno(self, geno, colnum):
        """extract_geno.R:8-12: column colnum (1-based) of M.ascii, served from the HBM-resident copy calcMMt left."""
        return self.r_api.extract_geno(geno["asciifileM"], colnum, dim_of_ascii_M=geno["dim_of_ascii_M"],
                                       device=self.device).astype(np.int64)


    def reshape(self, geno, indxNA):
        """AM.R:345-366 in VIEW mode: drops the individuals indxNA (1-based) from both genotype files without writing either; the
        returned geno names the views."""
        return reshape_geno(geno, indxNA, view=True, device=self.device)


class SpectralBackend(HipBackend):
    """The same loop with the scan in the eigenbasis of MM^T (include/eagle_hip.h section 1d; OPT-IN, needs the R-side change
    INTEGRATION.md describes): K = MM^T/max + 0.95 I is fixed for the whole run, so Z = Mt U is made once after calcMMt and
    every find_qtl is one HBM-bound pass over Z instead of an n x n quadratic form per marker.  Selects the markers the
    reference-shaped path selects (tests/test_am_driver.py)."""

    def __init__(self, device=0):
        super().__init__(device)
        self.lam = self.U = None
        self.L = None

    calcMMt_plain = HipBackend.calcMMt    # K alone: what AM(Zmat=) asks for, followed by prepare_z

    def prepare_z(self, geno, zmodel, availmemGb):
        """Repeated measures: Z~ = Mt (D^1/2 U~ / sqrt(d_max)) for U~ of D^1/2 K D^1/2 (host_model.ZModel), once per run."""
        self.lam = self.U = None
        n, self.L = geno["dim_of_ascii_M"]
        basis, _ = zmodel.spectral_basis()
        self.rcpp_api.spectral_prepare(geno["asciifileMt"], (self.L, n), basis, availmemGb, device=self.device)

    def calcMMt(self, geno, availmemGb, ncpu, selected_loci, quiet):
        MMt = super().calcMMt(geno, availmemGb, ncpu, selected_loci, quiet)
        self.lam, self.U = np.linalg.eigh(MMt)                       # the decomposition emma.REMLE needs anyway
        n, self.L = geno["dim_of_ascii_M"]
        self.rcpp_api.spectral_prepare(geno["asciifileMt"], (self.L, n), self.U, availmemGb, device=self.device)
        return MMt

    @property
    def eig(self):
        """(lam, U) of the last run's K, what r_api.SummaryAM(..., eig=) takes instead of its own eigh; None before a run."""
        return None if self.U is None else (self.lam, self.U)

    def find_qtl(self, geno, availmemGb, selected_loci, MMt, invMMt, best_ve, best_vg, currentX, ncpu, quiet, trait, Zmat=None):
        if Zmat is not None:   # a host_model.ZModel whose basis prepare_z made resident
            op = Zmat.spectral_operands(currentX, trait, best_ve, best_vg)
            res = self.rcpp_api.spectral_scan_weights(op["d"], op["Gy"], op["GX"], op["C"], op["c1"], best_vg, self.L, selected_loci,
                                                      device=self.device)
        else:
            res = self.rcpp_api.spectral_scan(self.lam, self.U.T @ currentX, self.U.T @ np.ravel(trait), best_ve, best_vg, self.L,
                                              selected_loci, device=self.device)
        with np.errstate(all="ignore"):
            tsq = res["a"].ravel() ** 2 / res["vara"].ravel()
        return int(np.flatnonzero(tsq == np.nanmax(tsq))[0]) + 1         # find_qtl.R:71-83


def reshape_geno(geno, indxNA, view=False, device=0):
    """AM.R:345-366: ReshapeM on the two files of `geno`, then geno names the results (<file>tmp) and carries the new dims.
    view=False writes the files (what a backend without its own `reshape` gets); view=True registers views on `device`."""
    from . import r_api
    newdims = r_api.ReshapeM(geno["asciifileM"], geno["asciifileMt"], indxNA, geno["dim_of_ascii_M"], view=view, device=device)
    return {"asciifileM": geno["asciifileM"] + "tmp", "asciifileMt": geno["asciifileMt"] + "tmp", "dim_of_ascii_M": newdims}


def AM(trait, X, geno, availmemGb=8, ncpu=1, maxit=20, quiet=True, backend=None, message=None, algebra=None, Zmat=None, gamma=1.0):
    """E/R/AM.R:320-475 for a trait vector and a ready design matrix X (n x q, intercept included).

    Individuals whose trait or any column of X is NaN are dropped (AM.R:320-329: an NA covariate makes the trait NA): from trait
    and X, and from the genotype files through backend.reshape(geno, indxNA) (AM.R:345-366; reshape_geno writing the files when
    the backend has no `reshape`).  A trait without NaN makes no such call.
    Returns dict(selected_loci = 1-based marker columns in order of selection, extBIC = list, ve, vg of the last fit, indxNA = the
    dropped rows, 1-based and largest first, and dim_of_ascii_M of the genotypes the loop ran on).
    selected_loci starts as [NA] exactly like AM.R:260, so the selected_loci masking never fires.

    Zmat: repeated measures (several records per genotyped individual), as r_api.ReadZmat's matrix or as ind_of_obs
    (r_api.zmat_index); trait and X then have one row per record -- see _AM_z.

    gamma: the weight on extBIC's model-space term (calc_extBIC); 1 is the reference's rule, a smaller value selects more loci.
    FPR4AM finds the gamma of a wanted false positive rate."""
    if Zmat is not None:
        return _AM_z(trait, X, geno, Zmat, availmemGb, ncpu, maxit, quiet, backend, message, algebra, gamma)
    backend = backend or HipBackend()
    if algebra is not None:  # "host" (LAPACK, the reference's placement) or "device" (rocSOLVER / the fp64 MFMA GEMM through the C ABI)
        host_model.set_algebra(algebra)
    say = message or (lambda *_: None)
    trait = np.asarray(trait, dtype=np.float64).ravel().copy()
    currentX = np.asarray(X, dtype=np.float64)
    trait[np.isnan(currentX).reshape(currentX.shape[0], -1).any(axis=1)] = np.nan   # AM.R:320-329
    from . import r_api
    indxNA = r_api.check_for_NA_in_trait(trait)                                     # AM.R:332
    if indxNA.size:                                                                  # AM.R:337-366
        keep = np.ones(trait.size, dtype=bool)
        keep[indxNA - 1] = False
        trait, currentX = trait[keep], currentX[keep]
        say(" The following rows are being removed from pheno due to missing data: %s" % " ".join(str(int(i)) for i in indxNA))
        geno = backend.reshape(geno, indxNA) if hasattr(backend, "reshape") else reshape_geno(geno, indxNA)
    nmarkers = geno["dim_of_ascii_M"][1]
    selected_loci = [np.nan]
    new_selected_locus = np.nan
    extBIC = []
    itnum, cont = 1, True
    MMt = invMMt = eig_L = None
    best = {}
    while cont:
        say("Iteration %d: Searching for most significant marker-trait association" % itnum)
        if not (isinstance(new_selected_locus, float) and math.isnan(new_selected_locus)):  # constructX.R:10-22
            currentX = np.column_stack([currentX, backend.extract_geno(geno, int(new_selected_locus)).astype(np.float64)])
        if itnum == 1:  # AM.R:414-422
            MMt = backend.calcMMt(geno, availmemGb, ncpu, np.array(selected_loci), quiet)
            invMMt = host_model._chol2inv(MMt)
            eig_L = emma_eigen_L_wo_Z(MMt)  # depends on MMt only; the reference recomputes it every iteration
        eig_R = emma_eigen_R_wo_Z(MMt, currentX)  # shared by REMLE and MLE of this iteration (same K, X)
        best = calcVC(trait, currentX, MMt, eig_R=eig_R)
        extBIC.append(calc_extBIC(trait, currentX, MMt, nmarkers, eig_L=eig_L, eig_R=eig_R, gamma=gamma))
        if int(np.flatnonzero(np.asarray(extBIC) == min(extBIC))[0]) == len(extBIC) - 1:  # AM.R:448
            new_selected_locus = backend.find_qtl(geno=geno, availmemGb=availmemGb, selected_loci=np.array(selected_loci), MMt=MMt,
                                                  invMMt=invMMt, best_ve=best["ve"], best_vg=best["vg"], currentX=currentX,
                                                  ncpu=ncpu, quiet=quiet, trait=trait)
            selected_loci.append(new_selected_locus)
        else:
            cont = False
        itnum += 1
        if itnum > maxit:  # AM.R:463-470
            cont = False
    # AM.R:476-499.  Stopped by maxit: every pick is reported (the in-loop report that drops the last pick is
    # overwritten by the one after the loop).  Stopped by extBIC: the last pick made extBIC worse and is dropped
    # together with its extBIC entry.
    picks = [int(v) for v in selected_loci[1:]]
    if itnum > maxit or len(selected_loci) <= 1:
        loci, ext = picks, list(extBIC)
    else:
        loci = picks[:-1]
        ext = [v for i, v in enumerate(extBIC) if i != len(selected_loci) - 1]
    return {"selected_loci": loci, "all_picks": picks, "extBIC": ext, "extBIC_trace": list(extBIC), "ve": best.get("ve"),
            "vg": best.get("vg"), "indxNA": indxNA, "dim_of_ascii_M": list(geno["dim_of_ascii_M"])}


def _AM_result(selected_loci, extBIC, itnum, maxit, best, indxNA, geno):
    """AM.R:476-499 (see AM())."""
    picks = [int(v) for v in selected_loci[1:]]
    if itnum > maxit or len(selected_loci) <= 1:
        loci, ext = picks, list(extBIC)
    else:
        loci = picks[:-1]
        ext = [v for i, v in enumerate(extBIC) if i != len(selected_loci) - 1]
    return {"selected_loci": loci, "all_picks": picks, "extBIC": ext, "extBIC_trace": list(extBIC), "ve": best.get("ve"),
            "vg": best.get("vg"), "indxNA": indxNA, "dim_of_ascii_M": list(geno["dim_of_ascii_M"])}


def _AM_z(trait, X, geno, Zmat, availmemGb, ncpu, maxit, quiet, backend, message, algebra, gamma=1.0):
    """AM() for y = X b + Z g + e: trait and X hold one row per RECORD, Zmat says whose record each is.

    Checks as check_inputs_mlam.R:122-145.  A record with NaN in trait or X is dropped (from trait, X and Z; the result's
    indxNA_obs, 1-based, largest first); an individual left without any record is dropped from the genotypes through
    backend.reshape (indxNA, as in AM(); the reference's complete == FALSE rule) and the others are renumbered.  Variance
    components and extBIC are emma_REMLE / emma_MLE with Z, n = the number of records; the scan runs over the t individuals with
    operands from Z^T P Z and Z^T P y (host_model.scan_operands_z), and a selected marker enters X as Z m_j.  The reference's own
    AM() cannot run this model (its .find_qtl takes no Z): the scan is this project's definition."""
    backend = backend or HipBackend()
    if algebra is not None:
        host_model.set_algebra(algebra)
    say = message or (lambda *_: None)
    trait = np.asarray(trait, dtype=np.float64).ravel().copy()
    currentX = np.asarray(X, dtype=np.float64)
    n_ind = int(geno["dim_of_ascii_M"][0])
    Zm = np.asarray(Zmat)
    if Zm.ndim == 2 and Zm.shape[1] != n_ind:                                        # check_inputs_mlam.R:124-130
        raise ValueError("Error: the number of columns specified in the Z matrix file is %d\n"
                         "       the number of rows specified in the genotype file is %d\n"
                         "       The number of columns in the Z matrix should be the same as the number of rows in the genotype file."
                         % (Zm.shape[1], n_ind))
    if Zm.shape[0] != trait.size:                                                    # check_inputs_mlam.R:139-145
        raise ValueError("Error: the number of rows specified in the Z matrix file is %d\n"
                         "       the number of rows specified in the phenotype file is %d\n"
                         "       The number of rows in the Z matrix file and phenotype file must be the same." % (Zm.shape[0], trait.size))
    if currentX.shape[0] != trait.size:
        raise ValueError("AM: %d rows of X for %d trait records" % (currentX.shape[0], trait.size))
    ind = as_ind_of_obs(Zm)
    if ind.min() < 0 or ind.max() >= n_ind:
        raise ValueError("AM: Zmat names individual %d, the genotypes hold %d" % (int(ind.max()) + 1, n_ind))
    currentX = currentX.reshape(trait.size, -1)
    trait[np.isnan(currentX).any(axis=1)] = np.nan                                   # AM.R:320-329, per record
    from . import r_api
    indxNA_obs = r_api.check_for_NA_in_trait(trait)
    if indxNA_obs.size:
        keep = np.ones(trait.size, dtype=bool)
        keep[indxNA_obs - 1] = False
        trait, currentX, ind = trait[keep], currentX[keep], ind[keep]
        say(" The following rows are being removed from pheno due to missing data: %s" % " ".join(str(int(i)) for i in indxNA_obs))
    has = np.bincount(ind, minlength=n_ind) > 0
    indxNA = (np.flatnonzero(~has) + 1)[::-1].copy()                                 # individuals, 1-based, largest first
    if indxNA.size:
        ind = (np.cumsum(has) - 1)[ind]
        say(" The following individuals have no record and are being removed from the genotypes: %s" % " ".join(str(int(i)) for i in indxNA))
        geno = backend.reshape(geno, indxNA) if hasattr(backend, "reshape") else reshape_geno(geno, indxNA)
    nmarkers = geno["dim_of_ascii_M"][1]
    selected_loci = [np.nan]
    new_selected_locus = np.nan
    extBIC = []
    itnum, cont = 1, True
    MMt = zm = None
    best = {}
    while cont:
        say("Iteration %d: Searching for most significant marker-trait association" % itnum)
        if not (isinstance(new_selected_locus, float) and math.isnan(new_selected_locus)):
            m = backend.extract_geno(geno, int(new_selected_locus)).astype(np.float64)
            currentX = np.column_stack([currentX, np.ravel(m)[ind]])                 # Z m_j
        if itnum == 1:
            MMt = getattr(backend, "calcMMt_plain", backend.calcMMt)(geno, availmemGb, ncpu, np.array(selected_loci), quiet)
            zm = host_model.ZModel(MMt, ind)                                         # the one eigh of the run
            if hasattr(backend, "prepare_z"):
                backend.prepare_z(geno, zm, availmemGb)
        best = calcVC(trait, currentX, MMt, zmodel=zm)
        extBIC.append(calc_extBIC(trait, currentX, MMt, nmarkers, zmodel=zm, gamma=gamma))
        if int(np.flatnonzero(np.asarray(extBIC) == min(extBIC))[0]) == len(extBIC) - 1:  # AM.R:448
            new_selected_locus = backend.find_qtl(geno=geno, availmemGb=availmemGb, selected_loci=np.array(selected_loci), MMt=MMt,
                                                  invMMt=None, best_ve=best["ve"], best_vg=best["vg"], currentX=currentX,
                                                  ncpu=ncpu, quiet=quiet, trait=trait, Zmat=zm)
            selected_loci.append(new_selected_locus)
        else:
            cont = False
        itnum += 1
        if itnum > maxit:
            cont = False
    out = _AM_result(selected_loci, extBIC, itnum, maxit, best, indxNA, geno)
    out["indxNA_obs"] = indxNA_obs
    return out


def AM_traits(Y, X, geno, availmemGb=8, maxit=20, quiet=True, message=None, algebra=None, device=0, Zmat=None, gamma=1.0):
    """AM() for the T columns of Y (n x T) with one design matrix X (n x q) on one genotype panel, in one run: calcMMt and
    lam, U = eigh(MM^T) once, Z = Mt U once (spectral_prepare), then the traits in lockstep -- each round one spectral_scan_traits
    call for every trait still running, and per trait emma_REMLE_eig / emma_MLE_eig in the eigenbasis (no n^3 work per trait or
    iteration).  Each trait follows AM()'s loop (stop rule AM.R:448, maxit, result assembly AM.R:476-499) and gets a dict with
    AM()'s keys.

    A row with NaN in ANY trait or in X is dropped for ALL traits (one VIEW reshape of the genotypes): with different NA patterns
    the result differs from separate AM() runs, which drop each trait's own NA rows only.  A pick adds its row of Z (U^T m_j,
    spectral_rows) to that trait's U^T X.

    Zmat (repeated measures) is not supported here: the per-trait EMMA in the eigenbasis and the batched kernel's own C would need
    AM(Zmat=)'s within-individual terms.  Run AM(Zmat=) per trait.

    gamma: the weight on extBIC's model-space term, as in AM()."""
    if Zmat is not None:
        raise NotImplementedError("AM_traits: Zmat (repeated measures) is not supported; run AM(Zmat=) for each trait")
    from . import r_api, rcpp_api
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y.reshape(Y.shape[0], -1).copy()
    currentX = np.asarray(X, dtype=np.float64).reshape(Y.shape[0], -1)
    T, q = Y.shape[1], currentX.shape[1]
    if q + maxit - 1 > 31:
        raise ValueError("AM_traits: q + maxit - 1 = %d fixed-effect columns in the last scan; the spectral scan takes at most 31"
                         % (q + maxit - 1))
    if algebra is not None:
        host_model.set_algebra(algebra)
    say = message or (lambda *_: None)
    na_row = np.isnan(Y).any(axis=1) | np.isnan(currentX).any(axis=1)
    indxNA = r_api.check_for_NA_in_trait(np.where(na_row, np.nan, 0.0))
    if indxNA.size:
        keep = ~na_row
        Y, currentX = Y[keep], currentX[keep]
        say(" The following rows are being removed from pheno due to missing data: %s" % " ".join(str(int(i)) for i in indxNA))
        geno = reshape_geno(geno, indxNA, view=True, device=device)
    n, nmarkers = geno["dim_of_ascii_M"]
    MMt = r_api.calcMMt(geno, availmemGb, 1, np.array([np.nan]), quiet, device=device)
    lam, U = host_model.algebra().eigh(MMt)
    lam = np.ascontiguousarray(lam)
    del MMt
    rcpp_api.spectral_prepare(geno["asciifileMt"], (nmarkers, n), U, availmemGb, device=device)
    UtY = U.T @ Y
    UtX0 = U.T @ currentX
    del U
    st = [{"UtX": UtX0, "sel": [np.nan], "ext": [], "best": {}, "itnum": 1, "cont": True} for _ in range(T)]
    while any(s["cont"] for s in st):
        active = [s for s in st if s["cont"]]
        scan = []
        for t, s in enumerate(st):
            if not s["cont"]:
                continue
            say("Trait %d, iteration %d: Searching for most significant marker-trait association" % (t + 1, s["itnum"]))
            r = emma_REMLE_eig(lam, s["UtX"], UtY[:, t])                                         # calcVC
            s["best"] = {"vg": r["vg"], "ve": r["ve"]}
            ml = emma_MLE_eig(lam, s["UtX"], UtY[:, t], llim=-100, ulim=100)                     # calc_extBIC
            k = s["UtX"].shape[1]
            s["ext"].append(-2 * ml["ML"] + (k + 1) * math.log(n) + 2 * gamma * _lchoose(nmarkers, k - 1))
            if int(np.flatnonzero(np.asarray(s["ext"]) == min(s["ext"]))[0]) == len(s["ext"]) - 1:   # AM.R:448
                scan.append(t)
            else:
                s["cont"] = False
        if scan:
            res = rcpp_api.spectral_scan_traits(lam, [st[t]["UtX"] for t in scan], UtY[:, scan], [st[t]["best"]["ve"] for t in scan],
                                                [st[t]["best"]["vg"] for t in scan], nmarkers, device=device)
            if np.any(res["index"] < 1):
                raise RuntimeError("AM_traits: every tsq of a scan is NaN")
            rows = rcpp_api.spectral_rows(res["index"] - 1, device=device)
            for j, t in enumerate(scan):
                st[t]["sel"].append(int(res["index"][j]))
                st[t]["UtX"] = np.column_stack([st[t]["UtX"], rows[:, j]])
        for s in active:
            s["itnum"] += 1
            if s["itnum"] > maxit:                                                                # AM.R:463-470
                s["cont"] = False
    out = []
    for s in st:   # AM.R:476-499, as in AM()
        picks = [int(v) for v in s["sel"][1:]]
        if s["itnum"] > maxit or len(s["sel"]) <= 1:
            loci, ext = picks, list(s["ext"])
        else:
            loci = picks[:-1]
            ext = [v for i, v in enumerate(s["ext"]) if i != len(s["sel"]) - 1]
        out.append({"selected_loci": loci, "all_picks": picks, "extBIC": ext, "extBIC_trace": list(s["ext"]), "ve": s["best"].get("ve"),
                    "vg": s["best"].get("vg"), "indxNA": indxNA, "dim_of_ascii_M": list(geno["dim_of_ascii_M"])})
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# FPR4AM: the gamma of a wanted false positive rate, from permutations of the trait.  Not in the reference
# tree (1.0.3); defined from the model.  For a permuted trait y_r AM() selects a (false) locus iff extBIC[1] < extBIC[0] (AM.R:448),
# which with q = ncol(X) and c = lchoose(L, q) - lchoose(L, q - 1) is gamma < gamma_star_r = (2 (ML1_r - ML0_r) - log n) / (2 c).
# ---------------------------------------------------------------------------------------------------------------------------
def fpr_curve(gamma_star, gammas):
    """FPR(gamma) = #{r : gamma_star_r > gamma} / R for every gamma of gammas: a step function that does not increase."""
    gs = np.asarray(gamma_star, dtype=np.float64).ravel()
    g = np.atleast_1d(np.asarray(gammas, dtype=np.float64))
    return (gs[None, :] > g.reshape(-1, 1)).sum(axis=1).reshape(g.shape) / gs.size


def choose_gamma(gamma_star, falseposrate):
    """The smallest gamma >= 0 with FPR(gamma) <= falseposrate: the k-th largest gamma_star, k = floor(falseposrate R) + 1, clipped
    below at 0.  k - 1 is found as the largest count m with m / R <= falseposrate, the comparison fpr_curve's values meet, so that
    a product falseposrate R that rounds below its integer value does not move k."""
    gs = np.asarray(gamma_star, dtype=np.float64).ravel()
    R = gs.size
    if R < 1 or not 0 < falseposrate < 1:
        raise ValueError("choose_gamma: at least one gamma_star and 0 < falseposrate < 1")
    m = int(math.floor(falseposrate * R))
    while (m + 1) / R <= falseposrate:
        m += 1
    while m / R > falseposrate:
        m -= 1
    return max(float(np.sort(gs)[::-1][m]), 0.0)


def _fpr_group(q):
    """Traits with q fixed-effect columns that one pass over Z scores (eagle_spectral_traits_passes)."""
    from . import rcpp_api
    g = 1
    while g < 128 and rcpp_api.spectral_traits_passes([q] * (g + 1)) == 1:
        g += 1
    return g


def FPR4AM(trait, X, geno, falseposrate=0.05, numreps=200, seed=101, availmemGb=8, quiet=True, message=None, algebra=None, device=0,
           eig=None, chunk=None):
    """The weight gamma on extBIC's model-space term at which AM(trait, X, geno, gamma=...) returns a false positive for the share
    falseposrate of traits without any association, estimated from numreps permutations of the trait.

    Rows with NaN in trait or X are dropped first (AM()'s rule, one VIEW reshape).  Permutation r is y[pi_r] with
    pi_r = rng.permutation(n), rng = numpy.random.default_rng(seed), drawn in order r = 0 .. numreps - 1; X and the genotypes stay.
    For each: the null fit on X (REML -> ve, vg; ML -> ML0), the scan's pick j_r, the ML fit on [X | m_j] (ML1) -- iterations 1 and 2
    of AM(y_r, X, geno, maxit=2) -- and gamma_star_r (above).  One calcMMt and one eigh (none with eig = (lam, U) of K, what
    SpectralBackend().eig holds), one spectral_prepare (none when rcpp_api.spectral_holds this Z), then per chunk of `chunk`
    permutations (default: whole column groups of the batched scan, as many as keep the stacked grid products within availmemGb / 8)
    one U^T Y, the batched EMMA, one spectral_scan_traits and one spectral_rows.  Nothing of size numreps x L exists.

    Returns dict(setgamma = choose_gamma(gamma_star, falseposrate), falseposrate = FPR(setgamma) achieved on these permutations,
    gamma_star, picks (1-based), tsqmax, ML0, ML1, ve, vg: numreps each; indxNA, seed, numreps).  setgamma may exceed 1.
    Permuting y against a structured K is an approximation under population structure (it breaks the trait's own covariance with K)."""
    from . import r_api, rcpp_api
    if not 0 < falseposrate < 1:
        raise ValueError("FPR4AM: falseposrate must lie strictly between 0 and 1, got %r" % (falseposrate,))
    numreps = int(numreps)
    if numreps < 1:
        raise ValueError("FPR4AM: numreps must be at least 1")
    y = np.asarray(trait, dtype=np.float64).ravel().copy()
    X0 = np.asarray(X, dtype=np.float64).reshape(y.size, -1)
    q = X0.shape[1]
    if q > 30:
        raise ValueError("FPR4AM: %d columns of X; at most 30 (the pick makes 31, the most the spectral scan takes)" % q)
    if chunk is not None and int(chunk) < 1:
        raise ValueError("FPR4AM: chunk must be at least 1")
    if algebra is not None:
        host_model.set_algebra(algebra)
    say = message or (lambda *_: None)
    y[np.isnan(X0).any(axis=1)] = np.nan                                             # AM.R:320-329
    indxNA = r_api.check_for_NA_in_trait(y)
    if indxNA.size:
        keep = ~np.isnan(y)
        y, X0 = y[keep], X0[keep]
        say(" The following rows are being removed from pheno due to missing data: %s" % " ".join(str(int(i)) for i in indxNA))
        geno = reshape_geno(geno, indxNA, view=True, device=device)
    n, L = (int(v) for v in geno["dim_of_ascii_M"])
    if y.size != n:
        raise ValueError("FPR4AM: %d trait records for %d genotyped individuals" % (y.size, n))
    la = host_model.algebra()
    if eig is None:
        MMt = r_api.calcMMt(geno, availmemGb, 1, np.array([np.nan]), quiet, device=device)
        lam, U = la.eigh(MMt)
        del MMt
    else:
        lam, U = eig
        if np.size(lam) != n or np.shape(U) != (n, n):
            raise ValueError("FPR4AM: eig holds %d eigenvalues, the genotypes %d individuals" % (np.size(lam), n))
    lam = np.ascontiguousarray(lam, dtype=np.float64).ravel()
    if not rcpp_api.spectral_holds(geno["asciifileMt"], U, device=device):
        rcpp_api.spectral_prepare(geno["asciifileMt"], (L, n), U, availmemGb, device=device)
    UtX = la.mm(U.T, X0)
    if chunk is None:
        g = _fpr_group(q)
        pairs = (q + 2) * (q + 3) // 2                                               # column products of [X | m_j | y]
        chunk = max(g, int(availmemGb * 2.0 ** 30 / 8 / (8.0 * n * pairs)) // g * g)
    chunk = int(chunk)
    c = _lchoose(L, q) - _lchoose(L, q - 1)
    rng = np.random.default_rng(seed)
    out = {k: np.zeros(numreps) for k in ("gamma_star", "tsqmax", "ML0", "ML1", "ve", "vg")}
    picks = np.zeros(numreps, dtype=np.int64)
    for r0 in range(0, numreps, chunk):
        r1 = min(r0 + chunk, numreps)
        say("Permutations %d to %d of %d" % (r0 + 1, r1, numreps))
        Yc = np.column_stack([y[rng.permutation(n)] for _ in range(r0, r1)])
        UtY = la.mm(U.T, Yc)
        vc = emma_REMLE_eig_batch(lam, UtX, UtY)                                     # calcVC of iteration 1
        ml0 = emma_MLE_eig_batch(lam, UtX, UtY, llim=-100, ulim=100)                 # calc_extBIC of iteration 1
        res = rcpp_api.spectral_scan_traits(lam, [UtX] * (r1 - r0), UtY, vc["ve"], vc["vg"], L, device=device)
        if np.any(res["index"] < 1):
            raise RuntimeError("FPR4AM: every tsq of a scan is NaN")
        uniq, inv = np.unique(np.asarray(res["index"], dtype=np.int64) - 1, return_inverse=True)
        rows = rcpp_api.spectral_rows(uniq, device=device)                           # U^T m_j of the distinct picks
        ml1 = emma_MLE_eig_batch(lam, UtX, UtY, last=rows[:, inv], llim=-100, ulim=100)   # calc_extBIC of iteration 2
        picks[r0:r1] = res["index"]
        for k, v in (("tsqmax", res["tsqmax"]), ("ML0", ml0["ML"]), ("ML1", ml1["ML"]), ("ve", vc["ve"]), ("vg", vc["vg"])):
            out[k][r0:r1] = v
    out["gamma_star"] = (2.0 * (out["ML1"] - out["ML0"]) - math.log(n)) / (2.0 * c)
    setgamma = choose_gamma(out["gamma_star"], falseposrate)
    out.update({"setgamma": setgamma, "falseposrate": float(fpr_curve(out["gamma_star"], setgamma)[0]), "picks": picks,
                "indxNA": indxNA, "seed": seed, "numreps": numreps})
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# SummaryAM (E/R/summary_am.R:78-221) in the eigenbasis of K.  Every model of summary_am.R uses K = MMt/max(MMt) + 0.95 I
# (.calcMMt, :140) or K'' = K/max(K) + 0.05 I (:186): with K = U diag(lam) U^T both share U, K'' having lam'' = lam/max(K) + 0.05.
# So with F = [X | m_j1 .. m_jk] (constructX, :131-137), Ft = U^T F and ut = U^T y:
#     H^-1 = U diag(D) U^T, D = 1/(vg lam + ve)   ->   F^T H^-1 F = Ft^T D Ft = A,   F^T H^-1 y = Ft^T D ut     (:149-151)
#     W_j = beta_j^2 / (A^-1)_jj                                                                                   (:155-159)
# and emma.REMLE (:143) / the k + 1 emma.MLE fits (:188, :205) are emma_REMLE_eig / emma_MLE_eig on leading column blocks of Ft.
# One eigh of K (none when the caller holds lam, U) instead of solve(H) and 2k + 3 n x n eigen() calls.
# ---------------------------------------------------------------------------------------------------------------------------
_SUMMARY_NONE = (" No significant marker-trait associations have been found by AM. \n", " Nothing to summarize. \n")   # :117-121


def _summary_names(q, xnames, map, L):
    """colnames of baseX (xnames; default "intercept", "X2", ...) and a function j (1-based) -> marker name: map's names (a
    sequence of L names, or a mapping with an "SNP" entry), by default M1 .. ML as summary_am.R:106-114."""
    xn = ["intercept"] + ["X%d" % j for j in range(2, q + 1)] if xnames is None else [str(v) for v in xnames]
    if len(xn) != q:
        raise ValueError("SummaryAM: %d xnames for %d columns of X" % (len(xn), q))
    if map is None:
        return xn, lambda j: "M%d" % j
    snp = list(map["SNP"]) if hasattr(map, "keys") else list(map)
    if len(snp) != L:
        raise ValueError("SummaryAM: map names %d markers, the genotypes hold %d" % (len(snp), L))
    return xn, lambda j: str(snp[j - 1])


def _summary_eig(lam, maxK, Ft, ut, q, names, say):
    """summary_am.R:142-217 from lam (eigenvalues of K), max(K), Ft = U^T [X | m_j1 .. m_jk] (n x (q + k)) and ut = U^T y."""
    lam = np.ascontiguousarray(lam, dtype=np.float64).ravel()
    n, p = Ft.shape
    eR = emma_REMLE_eig(lam, Ft, ut, llim=-100, ulim=100)                                         # :143
    D = 1.0 / (eR["vg"] * lam + eR["ve"])                                                          # :149-150
    FD = Ft * D[:, None]
    Ainv = np.linalg.inv(Ft.T @ FD)
    beta = Ainv @ (FD.T @ ut)                                                                      # :151
    W = beta * beta / np.diag(Ainv)                                                                # :157-159
    pval = 1.0 - chdtr(1, W)                                                                       # :160, 1 - pchisq(W, 1)
    say(" ~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~ \n")
    say("     Size and Significance of Effects in Final Model    \n")
    say(" ~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~ \n")
    say("%15s  %10s  %10s \n" % ("Name", "Additive effect", "p-value"))
    for nm, b, pv in zip(names, beta, pval):
        say("%15s  %10f         %.3E\n" % (nm, b, pv))
    say("\n\n\n")
    lam2 = lam / maxK + 0.05                                                                       # :186
    base = emma_MLE_eig(lam2, Ft[:, :q], ut, llim=-100, ulim=100)["ML"]                            # :188
    say(" ~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~ \n")
    say(" Proportion of Phenotype Variance Explained by Multiple-locus \n")
    say("             Association Mapping Model \n")
    say("  Marker loci which were found by AM() are added one at a time    \n")
    say(" ~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~ \n")
    say("   %15s      %10s \n" % ("Marker name", "Proportion"))
    rnames, rsq = [], []
    for k in range(q + 1, p + 1):                                                                  # :200-211
        full = emma_MLE_eig(lam2, Ft[:, :k], ut, llim=-100, ulim=100)["ML"]
        rsq.append(1.0 - math.exp(-2.0 / n * (full - base)))
        say("  %+15s          %.3f\n" % ("+  " + names[k - 1], rsq[-1]))
        rnames.append("+ " + names[k - 1])
    pval = [float(v) for v in pval]
    return {"pvalue": {"effects": list(names), "p_value": pval, "W": [float(v) for v in W]},
            "size": {"effect_names": list(names), "estimate": [float(v) for v in beta], "p_value": list(pval)},
            "R": {"Marker_name": rnames, "Prop_var_explained": rsq}}


def _summary_K(backend, geno, availmemGb, eig):
    """K by calcMMt with selected_loci = NA (summary_am.R:140; the masking never fires), max(K), and lam, U: eig
    when given, else one eigh of K."""
    n = geno["dim_of_ascii_M"][0]
    K = backend.calcMMt(geno, availmemGb, 1, np.array([np.nan]), True)
    maxK = float(np.max(K))
    if eig is None:
        lam, U = host_model.algebra().eigh(K)
    else:
        lam, U = eig
        if np.size(lam) != n or np.shape(U) != (n, n):
            raise ValueError("SummaryAM: eig holds %d eigenvalues, the genotypes %d individuals" % (np.size(lam), n))
    return maxK, np.ascontiguousarray(lam, dtype=np.float64).ravel(), U


def SummaryAM_traits(results, Y, X, geno, map=None, xnames=None, availmemGb=8, eig=None, backend=None, message=None, device=0):
    """r_api.SummaryAM for every entry of AM_traits(Y, X, geno)'s result, with one calcMMt and one eigh (none with eig=) for
    all traits.  The rows are AM_traits': a row with NaN in any trait or in X is dropped for all traits (backend.reshape, or
    reshape_geno writing files for a backend without one).  The marker columns of U^T F come from the resident Z (spectral_rows)
    when it was made from these genotypes with exactly this U -- the AM_traits run's context still open --, else from one
    host_model.algebra().mm over the union of all traits' picks.  Returns a list of SummaryAM results (None for a trait with no
    pick)."""
    from . import r_api, rcpp_api
    say = message or (lambda *_: None)
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y.reshape(Y.shape[0], -1)
    X = np.asarray(X, dtype=np.float64).reshape(Y.shape[0], -1)
    if len(results) != Y.shape[1]:
        raise ValueError("SummaryAM_traits: %d results for %d traits" % (len(results), Y.shape[1]))
    picks = [[int(j) for j in r["selected_loci"]] for r in results]
    if not any(picks):
        for _ in picks:
            for m in _SUMMARY_NONE:
                say(m)
        return [None] * len(picks)
    backend = backend or HipBackend(device)
    na_row = np.isnan(Y).any(axis=1) | np.isnan(X).any(axis=1)
    indxNA = r_api.check_for_NA_in_trait(np.where(na_row, np.nan, 0.0))
    if indxNA.size:
        Y, X = Y[~na_row], X[~na_row]
        geno = backend.reshape(geno, indxNA) if hasattr(backend, "reshape") else reshape_geno(geno, indxNA)
    n, L = geno["dim_of_ascii_M"]
    if Y.shape[0] != n:
        raise ValueError("SummaryAM_traits: %d trait records for %d genotyped individuals" % (Y.shape[0], n))
    q = X.shape[1]
    xn, mname = _summary_names(q, xnames, map, L)
    maxK, lam, U = _summary_K(backend, geno, availmemGb, eig)
    la = host_model.algebra()
    UtXY = la.mm(U.T, np.column_stack([X, Y]))
    union = sorted({j for pk in picks for j in pk})
    if rcpp_api.spectral_holds(geno["asciifileMt"], U, device=device):
        UtM = rcpp_api.spectral_rows(np.asarray(union) - 1, device=device)
    else:
        UtM = la.mm(U.T, np.column_stack([backend.extract_geno(geno, j).astype(np.float64) for j in union]))
    col = {j: i for i, j in enumerate(union)}
    out = []
    for t, pk in enumerate(picks):
        if not pk:
            for m in _SUMMARY_NONE:
                say(m)
            out.append(None)
            continue
        Ft = np.column_stack([UtXY[:, :q], UtM[:, [col[j] for j in pk]]])
        out.append(_summary_eig(lam, maxK, Ft, UtXY[:, q + t], q, xn + [mname(j) for j in pk], say))
    return out
