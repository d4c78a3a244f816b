"""The EMMA numerics of the AM() loop (am.py) -- host side, numpy/LAPACK: emma.REMLE / emma.MLE as the reference states them
(n x n eigen() per call), and the same profile likelihood in the eigenbasis of K for one trait, for T traits at once, and with a Z
matrix.  One bracket rule (_optimise), one zeroin, one likelihood (_z_fit / _z_ll / _z_dll) and one result dict (_emma_result)
serve them all.  am.py re-exports every name of this module; the reference line map is in its docstring.
"""
import math

import numpy as np

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


def _emma_result(key, LL=0, delta=0, va=0):
    """What every emma_* function returns, key = "REML" or "ML"; the defaults are a singular design's (emma_REMLE.R:28-30)."""
    return {key: LL, "delta": delta, "ve": va * delta, "vg": va}


def emma_REMLE(y, X, K, Z=None, ngrids=100, llim=-10, ulim=10, esp=1e-10, eig_R=None, zmodel=None):
    """Z: None, or the repeated-measures design as ind_of_obs (or the dense 0/1 matrix): the reduced form of _emma_z."""
    n, q = y.size, X.shape[1]
    if np.linalg.det(X.T @ X) == 0:
        return _emma_result("REML")
    if Z is not None or zmodel is not None:
        return _emma_result("REML", *_emma_z(y, X, K, Z, zmodel, ngrids, llim, ulim, esp, True))
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
    return _emma_result("REML", maxLL, maxdelta, maxva)


def emma_MLE(y, X, K, Z=None, ngrids=100, llim=-10, ulim=10, esp=1e-10, eig_L=None, eig_R=None, zmodel=None):
    n = y.size
    if np.linalg.det(X.T @ X) == 0:
        return _emma_result("ML")
    if Z is not None or zmodel is not None:
        return _emma_result("ML", *_emma_z(y, X, K, Z, zmodel, ngrids, llim, ulim, esp, False))
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
    return _emma_result("ML", maxLL, maxdelta, maxva)


# ---------------------------------------------------------------------------------------------------------------------------
# emma.REMLE / emma.MLE in the eigenbasis of K (K = U diag(lam) U^T, fixed for a whole run), the FaST-LMM identities: with
# Ut = U^T X, ut = U^T y, w_k = 1/(lam_k + delta), A = Ut^T W Ut, b = Ut^T W ut,
#     y^T P y = R = ut^T W ut - b^T A^-1 b,   P y = U r,  r = W (ut - Ut A^-1 b),
#     sum log(eig_R + delta) = sum log(lam + delta) + log det A - log det Ut^T Ut,   tr P = sum w - sum_k w_k^2 (Ut A^-1 Ut^T)_kk,
# so every likelihood evaluation costs O(n q^2) instead of the n^3 eigen() of S (K + I) S (emma_eigen_R_wo_Z).  The functions are
# equal in exact arithmetic to _reml_ll / _reml_dll / _ml_ll / _ml_dll; grid, bracket rule and zeroin are emma_REMLE's / emma_MLE's.
#
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
#
# One set of functions states both: the model without Z is Wn = None (no within-individual part) with n = t, where every Z term is an
# exact zero.
# ---------------------------------------------------------------------------------------------------------------------------
def _z_fit(lam, Ut, ut, Wn, delta):
    """w, W Ut, A, the W-weighted residual r, the within-individual residual sum of squares at beta (0 without Z) and R = y^T P y
    at one delta (R from the residual: no cancellation)."""
    q = Ut.shape[1]
    w = 1.0 / (lam + delta)
    Uw = Ut * w[:, None]
    A, b = Ut.T @ Uw, Uw.T @ ut
    if Wn is not None:
        A, b = A + Wn[:q, :q] / delta, b + Wn[:q, q] / delta
    beta = np.linalg.solve(A, b)
    e = ut - Ut @ beta
    rw = 0.0
    if Wn is not None:
        c = np.append(beta, -1.0)
        rw = max(float(c @ Wn @ c), 0.0)
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
    if reml:   # sum_k w_k^2 (Ut A^-1 Ut^T)_kk = tr(A^-1 Ut^T W^2 Ut), with Z plus the within-individual part
        trP -= np.sum(np.linalg.inv(A) * (Uw.T @ Uw if Wn is None else Uw.T @ Uw + Wn[:q, :q] / (d * d)))
    return 0.5 * ((n - q if reml else n) * (np.sum(r * r) + rw / (d * d)) / R - trP)


def _optimum(dLL, logdelta, llim, ulim, esp, lam, Ut, ut, Wn, n, reml, logdet_xtx):
    """From one trait's dLL/dlogdelta on the grid to (LL, delta, va) at the optimum: _optimise on the scalar likelihood."""
    maxdelta, maxLL = _optimise(dLL, logdelta, llim, ulim, esp, lambda ld: _z_ll(ld, lam, Ut, ut, Wn, n, reml, logdet_xtx),
                                lambda ld: _z_dll(ld, lam, Ut, ut, Wn, n, reml))
    return maxLL, maxdelta, _z_fit(lam, Ut, ut, Wn, maxdelta)[5] / (n - Ut.shape[1] if reml else n)


_grid_memo = []   # [(lam, delta, [W | W^2])]: the same lam and grids serve every trait and iteration of a run


def _grid_weights(lam, delta):
    for lm, dl, WW in _grid_memo:
        if lm is lam and np.array_equal(dl, delta):
            return WW
    Wg = 1.0 / (lam[:, None] + delta[None, :])
    WW = np.hstack([Wg, Wg * Wg])
    _grid_memo[:] = ([e for e in _grid_memo if e[0] is lam] + [(lam, delta, WW)])[-2:]
    return WW


# ---------------------------------------------------------------------------------------------------------------------------
# The grid for T traits at once (FPR4AM).  Trait t has the design [UtX | last[:, t]] (last = None: UtX
# alone, the null fits of a permutation study) and the trait column UtY[:, t].  The weights [W | W^2] depend on lam only, so the
# 101-point dLL grid of ALL traits is ONE product of the stacked (T (q+1)(q+2)/2) x n column products with them, through
# host_model.algebra().mm (the fp64 GEMM of the device with algebra="device"); bracket rule, zeroin and end-point rule then run
# per trait on the scalar functions (_optimum).  A single trait is T = 1 with numpy's own product: its fits stay on the host.
# ---------------------------------------------------------------------------------------------------------------------------
def _eig_grid_dll_batch(lam, B, delta, reml, mm):
    """dLL/dlogdelta on the whole grid for B = T x n x (q+1), trait t's [Ut_t | ut_t], T x m values from one GEMM (mm): the
    n x (q+1)(q+2)/2 products of row entries times the n x 2m weights [W | W^2], then (q+1) x (q+1) algebra per grid point."""
    T, n, q1 = B.shape
    q = q1 - 1
    iu, ju = np.triu_indices(q1)
    WW = _grid_weights(lam, delta)
    PT = np.ascontiguousarray((B[:, :, iu] * B[:, :, ju]).transpose(0, 2, 1)).reshape(T * iu.size, n)
    S = np.asarray(mm(PT, WW)).reshape(T, iu.size, -1)                           # (T (q+1)(q+2)/2) x 2m in one product
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


def _eig_grid_dll(lam, Ut, ut, delta, reml):
    return _eig_grid_dll_batch(lam, np.column_stack([Ut, ut])[None], delta, reml, np.matmul)[0]


def _emma_eig(lam, UtX, Uty, ngrids, llim, ulim, esp, reml):
    """-> (LL, delta, va), or () for a singular X^T X."""
    lam = np.asarray(lam, dtype=np.float64).ravel()
    Ut = np.asarray(UtX, dtype=np.float64).reshape(lam.size, -1)
    ut = np.asarray(Uty, dtype=np.float64).ravel()
    xtx = Ut.T @ Ut                                  # = X^T X (U orthogonal)
    if np.linalg.det(xtx) == 0:
        return ()
    logdelta, delta = _grid(ngrids, llim, ulim)
    dLL = _eig_grid_dll(lam, Ut, ut, delta, reml)
    return _optimum(dLL, logdelta, llim, ulim, esp, lam, Ut, ut, None, lam.size, reml, np.linalg.slogdet(xtx)[1])


def emma_REMLE_eig(lam, UtX, Uty, ngrids=100, llim=-10, ulim=10, esp=1e-10):
    """emma_REMLE(y, X, K) from lam, U = eigh(K): UtX = U^T X (n x q), Uty = U^T y.  No n^3 work."""
    return _emma_result("REML", *_emma_eig(lam, UtX, Uty, ngrids, llim, ulim, esp, True))


def emma_MLE_eig(lam, UtX, Uty, ngrids=100, llim=-10, ulim=10, esp=1e-10):
    """emma_MLE(y, X, K) from lam, U = eigh(K) (the xi of emma_MLE are lam)."""
    return _emma_result("ML", *_emma_eig(lam, UtX, Uty, ngrids, llim, ulim, esp, False))


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
    out = np.zeros((3, T))
    xtx = [Ut0.T @ Ut0] * T if last is None else [B[t, :, :q].T @ B[t, :, :q] for t in range(T)]    # = X_t^T X_t (U orthogonal)
    ok = [t for t in range(T) if np.linalg.det(xtx[t]) != 0]
    if not ok:
        return out
    logdelta, delta = _grid(ngrids, llim, ulim)
    dLL = _eig_grid_dll_batch(lam, B if len(ok) == T else B[ok], delta, reml, host_model.algebra().mm)
    for k, t in enumerate(ok):
        Ut, ut = np.ascontiguousarray(B[t, :, :q]), np.ascontiguousarray(B[t, :, q])
        out[:, t] = _optimum(dLL[k], logdelta, llim, ulim, esp, lam, Ut, ut, None, n, reml, np.linalg.slogdet(xtx[t])[1])
    return out


def emma_REMLE_eig_batch(lam, UtX, UtY, last=None, ngrids=100, llim=-10, ulim=10, esp=1e-10):
    """emma_REMLE_eig for the T columns of UtY (n x T): the design of trait t is UtX (n x q, shared), with last (n x T) given
    [UtX | last[:, t]].  Returns {"REML", "delta", "ve", "vg"} of arrays of length T."""
    return _emma_result("REML", *_emma_eig_batch(lam, UtX, UtY, last, ngrids, llim, ulim, esp, True))


def emma_MLE_eig_batch(lam, UtX, UtY, last=None, ngrids=100, llim=-10, ulim=10, esp=1e-10):
    """emma_MLE_eig for the T columns of UtY; arguments as emma_REMLE_eig_batch.  Returns {"ML", "delta", "ve", "vg"}."""
    return _emma_result("ML", *_emma_eig_batch(lam, UtX, UtY, last, ngrids, llim, ulim, esp, False))


def as_ind_of_obs(Z):
    """ind_of_obs (0-based int64) from either form of a Z matrix: the vector itself, or the dense n_obs x t 0/1 matrix."""
    Z = np.asarray(Z)
    if Z.ndim == 2:
        from . import r_api
        return r_api.zmat_index(Z)
    return Z.astype(np.int64).ravel()


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
    return _optimum(dLL, logdelta, llim, ulim, esp, lam, Ut, ut, Wn, n, reml, logdet_xtx)
