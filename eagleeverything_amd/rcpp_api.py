"""Host-side mirror of the reference's exported C++ functions, over the C ABI of libeaglehip.so.

Same names, argument order and error behaviour as the functions registered in
E/src/RcppExports.cpp:154-170 (E/ = MyPackage/Eagle/ of the reference), so a parity test reads like a
call into the reference:

    ReadBlock(asciifname, start_row, numcols, numrows_in_block)                          RcppExports.cpp:9
    calculateMMt_rcpp(f_name_ascii, max_memory_in_Gbytes, num_cores, selected_loci, dims, quiet, message)   :37
    calculate_a_and_vara_rcpp(f_name_ascii, selected_loci, inv_MMt_sqrt, dim_reduced_vara,
                              max_memory_in_Gbytes, dims, a, quiet, message)             :54
    calculate_reduced_a_rcpp(f_name_ascii, varG, P, y, max_memory_in_Gbytes, dims, selected_loci, quiet, message)  :73
    extract_geno_rcpp(f_name_ascii, max_memory_in_Gbytes, selected_locus, dims)                                  :129

R matrices are column-major; numpy arrays are converted to Fortran order on the way in and come back so.
NA is numpy.nan.  Every call runs on the GPU; nothing here computes.
"""
import ctypes as C
import os

import numpy as np

from . import _lib, host_model
from ._lib import EagleError, c_dp, c_lp

_ctx = {}
_callbacks = {}
_spectral_n = {}   # device -> n of the Z its last spectral_prepare made
_spectral_key = {}  # device -> (Mt file name, content key of U) of that Z: what spectral_holds compares against


def context(device=0):
    """The eagle_ctx of `device` (opened on first use; fails loudly without a gfx950 device).  `device` may be a tuple of
    device numbers: ONE context that shards every call's markers over those GPUs (eagle_open_devices; the reference's unused
    AM(..., ngpu) hook, E/R/AM.R:185-196) -- pass the same tuple as `device=` to the functions below."""
    if device not in _ctx:
        L = _lib.load()
        if isinstance(device, tuple):
            arr = (C.c_int * len(device))(*[int(d) for d in device])
            h = L.eagle_open_devices(arr, len(device))
        else:
            h = L.eagle_open(int(device))
        if not h:
            raise EagleError(-6, L.eagle_open_error().decode())
        _ctx[device] = h
    return _ctx[device]


def close_all():
    L = _lib.load()
    for h in _ctx.values():
        L.eagle_close(h)
    _ctx.clear()
    _views.clear()
    _callbacks.clear()
    _spectral_n.clear()
    _spectral_key.clear()


def _check(ctx, rc, soft_ok=False):
    if rc < 0 or (rc > 0 and not soft_ok):
        raise EagleError(rc, _lib.load().eagle_last_error(ctx).decode())
    return rc


def _dp(a):
    return a.ctypes.data_as(c_dp)


def _f64F(a):
    return np.require(np.asarray(a, dtype=np.float64), requirements=["F", "ALIGNED"])


def _sel(selected_loci):
    s = np.atleast_1d(np.asarray(selected_loci, dtype=np.float64)).copy()
    return s, _dp(s), s.size


def _dims(dims):
    d = (C.c_long * 2)(int(dims[0]), int(dims[1]))
    return d


def _set_message(ctx, message):
    L = _lib.load()
    if message is None:
        L.eagle_set_message_callback(ctx, C.cast(None, _lib.MESSAGE_FN), None)
        _callbacks.pop(ctx, None)
    else:
        cb = _lib.MESSAGE_FN(lambda text, user: message(text.decode()))
        _callbacks[ctx] = cb  # keep alive
        L.eagle_set_message_callback(ctx, cb, None)


def device_info(device=0):
    L = _lib.load()
    ctx = context(device)
    arch = C.create_string_buffer(64)
    cu = C.c_int()
    hbm = C.c_int64()
    _check(ctx, L.eagle_device_info(ctx, arch, 64, C.byref(cu), C.byref(hbm)))
    return {"arch": arch.value.decode(), "cu_count": cu.value, "hbm_bytes": hbm.value}


def set_scan_mode(mode, device=0):
    """1 (default) = int8-slice vara kernel, 0 = fp64 MFMA vara kernel."""
    ctx = context(device)
    _check(ctx, _lib.load().eagle_set_scan_mode(ctx, int(mode)))


def set_scan_slices(nslices, device=0):
    """Base-256 digits of W used by the int8-slice kernel (1..8, default 7)."""
    ctx = context(device)
    _check(ctx, _lib.load().eagle_set_scan_slices(ctx, int(nslices)))


def set_scan_rounding(stochastic, device=0):
    """0 (default) = digits of W rounded to nearest (guaranteed bound); 1 = stochastic rounding (probabilistic certificate,
    failure probability < 1e-30 per marker, one digit fewer)."""
    ctx = context(device)
    _check(ctx, _lib.load().eagle_set_scan_rounding(ctx, int(stochastic)))


def set_scan_budget(relative_budget, device=0):
    """Relative digit budget of the int8 scan.  A context whose budget was never set tries 1e-7 first and falls back to 5e-7 (half of the
    path's 1e-6 tolerance); a value given here becomes THE budget, 0 restores that default policy.  The certificate sends every marker
    whose own bound exceeds 1.8 x the budget it enforces (last_scan_enforced) to the fp64 kernel."""
    ctx = context(device)
    _check(ctx, _lib.load().eagle_set_scan_budget(ctx, float(relative_budget)))


def last_scan_budget(device=0):
    """(budget in force for the last digit-slice scan, level of the spectral bound that took the digit off, error bound of an int8-made W)."""
    ctx = context(device)
    b, lv, we = C.c_double(), C.c_int(), C.c_double()
    _check(ctx, _lib.load().eagle_last_scan_budget(ctx, C.byref(b), C.byref(lv), C.byref(we)))
    return b.value, lv.value, we.value


def last_scan_enforced(device=0):
    """(budget the certificate of the last digit-slice scan enforced per marker, markers over the tight threshold): the budget in force, or
    the default behind a tight one when more than 512 markers of the whole scan missed the tight threshold (eagle_last_scan_enforced)."""
    ctx = context(device)
    b, nt = C.c_double(), C.c_long()
    _check(ctx, _lib.load().eagle_last_scan_enforced(ctx, C.byref(b), C.byref(nt)))
    return b.value, nt.value


def prepare_scan(n, L, device=0):
    """Start the allocation of the scan's device arena on a background thread (eagle_prepare_scan; calculateMMt_rcpp does it by itself)."""
    ctx = context(device)
    _check(ctx, _lib.load().eagle_prepare_scan(ctx, int(n), int(L)))


def set_w_mode(mode, device=0):
    """Which engine forms W = S (V S) for a digit-slice scan: 1 (default) = int8 digit slices from 4,096 padded individuals up, 0 = always
    the fp64 GEMM, 2 = int8 at any size (eagle_set_w_mode, csrc/eagle_w8.hip)."""
    ctx = context(device)
    _check(ctx, _lib.load().eagle_set_w_mode(ctx, int(mode)))


class _WInfo(C.Structure):
    _fields_ = [("int8", C.c_int), ("declined", C.c_int), ("k1", C.c_int), ("T1", C.c_int), ("pairs1", C.c_int), ("k2", C.c_int), ("T2", C.c_int),
                ("pairs2", C.c_int), ("eta", C.c_double), ("eta_x", C.c_double), ("target", C.c_double), ("mean_diag", C.c_double),
                ("asym_term", C.c_double), ("pipelined", C.c_int), ("pad", C.c_int)]


def last_w_info(device=0):
    """eagle_last_w_info as a dict: which engine formed the W of the last scan on this device, its configuration and error bound."""
    ctx = context(device)
    i = _WInfo()
    _check(ctx, _lib.load().eagle_last_w_info(ctx, C.byref(i)))
    return {k: getattr(i, k) for k, _ in _WInfo._fields_}


def drop_cache(device=0):
    _lib.load().eagle_drop_cache(context(device))


def ReadBlock(asciifname, start_row, numcols, numrows_in_block, device=0):
    L = _lib.load()
    ctx = context(device)
    out = np.zeros((int(numrows_in_block), int(numcols)), dtype=np.float64, order="F")
    _check(ctx, L.eagle_read_block(ctx, os.fsencode(asciifname), int(start_row), int(numcols), int(numrows_in_block),
                                   _dp(out)))
    return out


def calculateMMt_rcpp(f_name_ascii, max_memory_in_Gbytes, num_cores, selected_loci, dims, quiet=True, message=None,
                      device=0):
    L = _lib.load()
    ctx = context(device)
    _set_message(ctx, message)
    n = int(dims[0])
    s, sp, ns = _sel(selected_loci)
    out = np.zeros((n, n), dtype=np.float64, order="F")
    _check(ctx, L.eagle_calculateMMt(ctx, os.fsencode(f_name_ascii), float(max_memory_in_Gbytes), int(num_cores), sp, ns,
                                     _dims(dims), int(bool(quiet)), _dp(out)))
    return out


def calculate_a_and_vara_rcpp(f_name_ascii, selected_loci, inv_MMt_sqrt, dim_reduced_vara, max_memory_in_Gbytes, dims,
                              a, quiet=True, message=None, device=0):
    L = _lib.load()
    ctx = context(device)
    _set_message(ctx, message)
    Lm, n = int(dims[0]), int(dims[1])
    S = _f64F(inv_MMt_sqrt)
    V = _f64F(dim_reduced_vara)
    ah = _f64F(np.ravel(a))
    if S.shape != (n, n) or V.shape != (n, n) or ah.size != n:
        raise ValueError("inv_MMt_sqrt / dim_reduced_vara must be n x n and a of length n")
    s, sp, ns = _sel(selected_loci)
    a_out = np.zeros(Lm)
    v_out = np.zeros(Lm)
    rc = _check(ctx, L.eagle_calculate_a_and_vara(ctx, os.fsencode(f_name_ascii), sp, ns, _dp(S), _dp(V),
                                                  float(max_memory_in_Gbytes), _dims(dims), _dp(ah), int(bool(quiet)),
                                                  _dp(a_out), _dp(v_out)), soft_ok=True)
    if rc == 1:  # List(a = 0, vara = 0), calculate_a_and_vara_rcpp.cpp:141-142
        return {"a": np.zeros(1), "vara": np.zeros(1)}
    return {"a": a_out.reshape(Lm, 1), "vara": v_out.reshape(Lm, 1)}


def scan_with_W(f_name_ascii, selected_loci, W, v, max_memory_in_Gbytes, dims, quiet=True, message=None, device=0):
    """eagle_scan_with_W: the scan of calculate_a_and_vara_rcpp with W = S V S and v = S a_hat ready-made (inside AM():
    W = varG^2 P, v = varG P y; no n^3 product).  Not a symbol of the reference; an R-side shortcut."""
    L = _lib.load()
    ctx = context(device)
    _set_message(ctx, message)
    Lm, n = int(dims[0]), int(dims[1])
    Wm = _f64F(W)
    vv = _f64F(np.ravel(v))
    if Wm.shape != (n, n) or vv.size != n:
        raise ValueError("W must be n x n and v of length n")
    s, sp, ns = _sel(selected_loci)
    a_out = np.zeros(Lm)
    v_out = np.zeros(Lm)
    _check(ctx, L.eagle_scan_with_W(ctx, os.fsencode(f_name_ascii), sp, ns, _dp(Wm), _dp(vv), float(max_memory_in_Gbytes), _dims(dims),
                                    int(bool(quiet)), _dp(a_out), _dp(v_out)))
    return {"a": a_out.reshape(Lm, 1), "vara": v_out.reshape(Lm, 1)}


def spectral_prepare(f_name_ascii, dims, U, max_memory_in_Gbytes=8.0, device=0):
    """eagle_spectral_prepare: Z = Mt U once per AM() run (dims = (L, n) of Mt.ascii, U = eigenvectors of the normalised MM^T)."""
    L = _lib.load()
    ctx = context(device)
    Um = _f64F(U)
    n = int(dims[1])
    if Um.shape != (n, n):
        raise ValueError("U must be n x n")
    _spectral_n.pop(device, None)
    _spectral_key.pop(device, None)
    _check(ctx, L.eagle_spectral_prepare(ctx, os.fsencode(f_name_ascii), _dims(dims), _dp(Um), float(max_memory_in_Gbytes)))
    _spectral_n[device] = n
    _spectral_key[device] = (str(f_name_ascii), host_model._content_key(Um))


def spectral_holds(f_name_ascii, U, device=0):
    """True when `device`'s resident Z is Mt U for this Mt file and exactly this U (same bytes), so that spectral_rows(j) is
    U^T m_j.  Opens no context."""
    key = _spectral_key.get(device)
    return key is not None and key[0] == str(f_name_ascii) and key[1] == host_model._content_key(_f64F(U))


def spectral_scan(lam, UtX, Uty, varE, varG, n_markers, selected_loci=np.nan, device=0):
    """eagle_spectral_scan: a and vara of every marker from one pass over Z (see include/eagle_hip.h section 1d)."""
    L = _lib.load()
    ctx = context(device)
    lam = _f64F(np.ravel(lam))
    UtX = _f64F(np.atleast_2d(UtX).reshape(lam.size, -1))
    Uty = _f64F(np.ravel(Uty))
    p = UtX.shape[1]
    s, sp, ns = _sel(selected_loci)
    a_out = np.zeros(int(n_markers))
    v_out = np.zeros(int(n_markers))
    _check(ctx, L.eagle_spectral_scan(ctx, _dp(lam), _dp(UtX), _dp(Uty), p, float(varE), float(varG), sp, ns, _dp(a_out), _dp(v_out)))
    return {"a": a_out.reshape(-1, 1), "vara": v_out.reshape(-1, 1)}


def spectral_scan_weights(d, Gy, GX, C, c1, varG, n_markers, selected_loci=np.nan, device=0):
    """eagle_spectral_scan_weights: the pass of spectral_scan with caller-made operands (include/eagle_hip.h section 1d):
    a_i = varG (z_i . Gy - q_i . c1), vara_i = varG^2 (sum_k z_ik^2 d_k - q_i^T C q_i), q_i = z_i^T GX."""
    L = _lib.load()
    ctx = context(device)
    d = _f64F(np.ravel(d))
    n = _spectral_n.get(device, 0)
    GX = _f64F(np.atleast_2d(GX).reshape(d.size, -1))
    Gy = _f64F(np.ravel(Gy))
    p = GX.shape[1]
    Cm = _f64F(np.asarray(C, dtype=np.float64).reshape(p, p))
    c1 = _f64F(np.ravel(c1))
    if d.size != n or Gy.size != n or c1.size != p:
        raise ValueError("spectral_scan_weights: d, Gy of length n = %d (the resident Z), GX n x p, C p x p, c1 of length p" % n)
    s, sp, ns = _sel(selected_loci)
    a_out = np.zeros(int(n_markers))
    v_out = np.zeros(int(n_markers))
    _check(ctx, L.eagle_spectral_scan_weights(ctx, _dp(d), _dp(Gy), _dp(GX), p, _dp(Cm), _dp(c1), float(varG), sp, ns, _dp(a_out),
                                              _dp(v_out)))
    return {"a": a_out.reshape(-1, 1), "vara": v_out.reshape(-1, 1)}


def spectral_traits_passes(p):
    """eagle_spectral_traits_passes: passes over Z one spectral_scan_traits call makes for traits with these p[t] columns."""
    pv = np.ascontiguousarray(np.atleast_1d(p), dtype=np.int64)
    rc = _lib.load().eagle_spectral_traits_passes(pv.size, pv.ctypes.data_as(c_lp))
    if rc < 0:
        raise ValueError("1 <= p[t] <= 31 and at least one trait")
    return rc


def _cols(a, n):
    a = np.asarray(a, dtype=np.float64)
    return _f64F(a.reshape(n, -1) if a.size else np.zeros((n, 0)))


def spectral_scan_traits(lam, UtX_list, UtY, varE, varG, n_markers, full=False, device=0):
    """eagle_spectral_scan_traits: T traits from as few passes over Z as the column groups allow (include/eagle_hip.h section 1d).
    UtX_list: T arrays n x p_t, UtY: n x T, varE / varG: T each.  Returns index (T, 1-based arg-max of tsq, 0 = every tsq NaN) and
    tsqmax (T); with full=True also a and vara (n_markers x T)."""
    L = _lib.load()
    ctx = context(device)
    lam = _f64F(np.ravel(lam))
    n = lam.size
    UtY = _cols(UtY, n)
    T = UtY.shape[1]
    UtX = [_cols(x, n) for x in UtX_list]
    if len(UtX) != T:
        raise ValueError("one U^T X per trait")
    p = np.array([x.shape[1] for x in UtX], dtype=np.int64)
    ptrs = (c_dp * max(T, 1))(*[_dp(x) for x in UtX])
    vE = np.ascontiguousarray(np.broadcast_to(np.asarray(varE, dtype=np.float64), (T,)))
    vG = np.ascontiguousarray(np.broadcast_to(np.asarray(varG, dtype=np.float64), (T,)))
    idx = np.zeros(max(T, 1), dtype=np.int64)
    mx = np.zeros(max(T, 1))
    a_out = np.zeros((int(n_markers), T), order="F") if full else None
    v_out = np.zeros((int(n_markers), T), order="F") if full else None
    _check(ctx, L.eagle_spectral_scan_traits(ctx, T, _dp(lam), ptrs, p.ctypes.data_as(c_lp), _dp(UtY), _dp(vE), _dp(vG),
                                             _dp(a_out) if full else None, _dp(v_out) if full else None,
                                             idx.ctypes.data_as(c_lp), _dp(mx)))
    res = {"index": idx[:T], "tsqmax": mx[:T]}
    if full:
        res["a"], res["vara"] = a_out, v_out
    return res


def spectral_rows(idx, device=0):
    """eagle_spectral_rows: U^T m_j of the markers idx (0-based) from the resident Z, n x k."""
    L = _lib.load()
    ctx = context(device)
    iv = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int64)
    n = _spectral_n.get(device, 0)
    out = np.zeros((n, iv.size), order="F")
    _check(ctx, L.eagle_spectral_rows(ctx, iv.ctypes.data_as(c_lp), iv.size, _dp(out)))
    return out


LMM_MAX_COVARIATES = 14


def spectral_lmm(lam, UtX, Uty, reml=True, theta0=0.0, tol=1e-10, max_iter=50, idx=None, n_markers=None, device=0):
    """eagle_spectral_lmm: the exact mixed-model test of include/eagle_hip.h section 1d' on the resident Z -> (stat (k, 5) = gamma, se,
    delta, vg, ll; info (k, 2) = code, iterations).  lam (n), UtX (n x c, 1 <= c <= 14, the intercept column included), Uty (n);
    theta0 = ln delta of the null fit.  idx: 0-based markers, the outputs in list order; None: all n_markers markers of the prepare."""
    lam = _f64F(np.ravel(lam))
    n = lam.size
    UtX = np.asarray(UtX, dtype=np.float64)
    if UtX.ndim == 1:
        UtX = UtX[:, None]
    Uty = _f64F(np.ravel(Uty))
    if UtX.ndim != 2 or UtX.shape[0] != n or not 1 <= UtX.shape[1] <= LMM_MAX_COVARIATES or Uty.size != n:
        raise ValueError("spectral_lmm: lam, Uty of length n and UtX (n, c) with 1 <= c <= %d" % LMM_MAX_COVARIATES)
    if not (np.all(np.isfinite(lam)) and np.all(np.isfinite(UtX)) and np.all(np.isfinite(Uty))):
        raise ValueError("spectral_lmm: a non-finite operand")
    if not (0.0 < float(tol) < 1.0) or int(max_iter) != max_iter or not 0 <= int(max_iter) <= 1000 or not np.isfinite(float(theta0)):
        raise ValueError("spectral_lmm: tol in (0, 1), max_iter an integer in [0, 1000], theta0 finite")
    if idx is None:
        if n_markers is None or int(n_markers) < 1:
            raise ValueError("spectral_lmm: n_markers (the markers of the prepare) is needed without idx")
        iv, k, ip = None, int(n_markers), None
    else:
        iv = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int64)
        if iv.ndim != 1 or (iv.size and iv.min() < 0):
            raise ValueError("spectral_lmm: idx must be a list of 0-based markers")
        k, ip = iv.size, iv.ctypes.data_as(c_lp)
    UtX = _f64F(UtX)
    L = _lib.load()
    ctx = context(device)
    stat = np.full((max(k, 1), 5), np.nan)
    info = np.zeros((max(k, 1), 2), dtype=np.int32)
    _check(ctx, L.eagle_spectral_lmm(ctx, _dp(lam), _dp(UtX), _dp(Uty), UtX.shape[1], int(bool(reml)), float(theta0), float(tol), int(max_iter),
                                     ip, k, _dp(stat), info.ctypes.data_as(C.POINTER(C.c_int32))))
    return stat[:k], info[:k]


SETTEST_MAX_MARKERS = 64


def settest_csr(sets, omega=None):
    """(set_ptr (k + 1), set_idx (nnz), omega (nnz)) int64 / int64 / fp64 of `sets`, a list of 1-D arrays of 0-based markers, and
    `omega`: None (every weight 1), a list of arrays shaped like the sets, or one flat array of nnz weights in CSR order."""
    idx = [np.ascontiguousarray(np.atleast_1d(s), dtype=np.int64) for s in sets]
    if any(s.ndim != 1 for s in idx):
        raise ValueError("settest: every set must be a 1-D list of 0-based markers")
    ptr = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum([s.size for s in idx], out=ptr[1:])
    flat = np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)
    if omega is None:
        w = np.ones(flat.size)
    elif isinstance(omega, (list, tuple)):
        if len(omega) != len(idx) or any(np.size(a) != s.size for a, s in zip(omega, idx)):
            raise ValueError("settest: one weight per marker of every set")
        w = np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in omega]) if idx else np.zeros(0)
    else:
        w = np.ascontiguousarray(np.ravel(omega), dtype=np.float64)
        if w.size != flat.size:
            raise ValueError("settest: one weight per marker of every set")
    return ptr, np.ascontiguousarray(flat), np.ascontiguousarray(w, dtype=np.float64)


def spectral_settest(lam, UtX, Uty, varE, varG, sets, omega=None, scores=False, cov=False, device=0):
    """eagle_spectral_settest: burden and SKAT statistics of marker sets on the resident Z (include/eagle_hip.h section 1d'') ->
    {"stat" (k, 7) = Q, Ub, Vb, c_1 .. c_4; "info" (k, 2) = code, markers used} and, with scores=True, "score": a list of k arrays
    (s_j of every set), with cov=True, "cov": a list of k symmetric (m, m) arrays (Phi).  lam (n), UtX (n x c, 1 <= c <= 14, the
    intercept column included), Uty (n), the null model's varE and varG; sets, omega: as settest_csr takes them (1 to
    SETTEST_MAX_MARKERS markers per set, weights finite and >= 0)."""
    lam = _f64F(np.ravel(lam))
    n = lam.size
    UtX = np.asarray(UtX, dtype=np.float64)
    if UtX.ndim == 1:
        UtX = UtX[:, None]
    Uty = _f64F(np.ravel(Uty))
    if UtX.ndim != 2 or UtX.shape[0] != n or not 1 <= UtX.shape[1] <= LMM_MAX_COVARIATES or Uty.size != n:
        raise ValueError("spectral_settest: lam, Uty of length n and UtX (n, c) with 1 <= c <= %d" % LMM_MAX_COVARIATES)
    if not (np.all(np.isfinite(lam)) and np.all(np.isfinite(UtX)) and np.all(np.isfinite(Uty)) and np.isfinite(float(varE))
            and np.isfinite(float(varG))):
        raise ValueError("spectral_settest: a non-finite operand")
    ptr, idx, w = settest_csr(sets, omega)
    m = np.diff(ptr)
    if m.size and (m.min() < 1 or m.max() > SETTEST_MAX_MARKERS):
        raise ValueError("spectral_settest: every set must hold 1 to %d markers" % SETTEST_MAX_MARKERS)
    if idx.size and idx.min() < 0:
        raise ValueError("spectral_settest: the sets hold 0-based markers")
    if not (np.all(np.isfinite(w)) and np.all(w >= 0.0)):
        raise ValueError("spectral_settest: the weights must be finite and >= 0")
    UtX = _f64F(UtX)
    k = m.size
    L = _lib.load()
    ctx = context(device)
    stat = np.full((max(k, 1), 7), np.nan)
    info = np.zeros((max(k, 1), 2), dtype=np.int32)
    sc = np.zeros(max(idx.size, 1)) if scores else None
    cv = np.zeros(max(int(np.sum(m * m)), 1)) if cov else None
    _check(ctx, L.eagle_spectral_settest(ctx, _dp(lam), _dp(UtX), _dp(Uty), UtX.shape[1], float(varE), float(varG), k, ptr.ctypes.data_as(c_lp),
                                         idx.ctypes.data_as(c_lp) if idx.size else np.zeros(1, dtype=np.int64).ctypes.data_as(c_lp),
                                         _dp(w) if w.size else _dp(np.zeros(1)), _dp(stat), info.ctypes.data_as(C.POINTER(C.c_int32)),
                                         _dp(sc) if scores else None, _dp(cv) if cov else None))
    out = {"stat": stat[:k], "info": info[:k]}
    if scores:
        out["score"] = [sc[ptr[o]:ptr[o + 1]].copy() for o in range(k)]
    if cov:
        off = np.concatenate([[0], np.cumsum(m * m)])
        out["cov"] = [cv[off[o]:off[o + 1]].reshape(m[o], m[o]).copy() for o in range(k)]
    return out


def calculate_reduced_a_rcpp(f_name_ascii, varG, P, y, max_memory_in_Gbytes, dims, selected_loci, quiet=True,
                             message=None, device=0):
    L = _lib.load()
    ctx = context(device)
    _set_message(ctx, message)
    n, Lm = int(dims[0]), int(dims[1])
    Pm = _f64F(P)
    yv = _f64F(np.ravel(y))
    s, sp, ns = _sel(selected_loci)
    out = np.zeros(Lm)
    rc = _check(ctx, L.eagle_calculate_reduced_a(ctx, os.fsencode(f_name_ascii), float(varG), _dp(Pm), _dp(yv),
                                                 float(max_memory_in_Gbytes), _dims(dims), sp, ns, int(bool(quiet)),
                                                 _dp(out)), soft_ok=True)
    if rc == 1:  # 1 x 1 zero matrix, calculate_reduced_a_rcpp.cpp:94-103
        return np.zeros((1, 1))
    return out.reshape(Lm, 1)


def extract_geno_rcpp(f_name_ascii, max_memory_in_Gbytes, selected_locus, dims, device=0):
    """E/src/extract_geno_rcpp.cpp:16-89: column selected_locus (0-based) of M.ascii as int32 -1/0/1."""
    L = _lib.load()
    ctx = context(device)
    n = int(dims[0])
    out = np.zeros(n, dtype=np.int32)
    _check(ctx, L.eagle_extract_geno(ctx, os.fsencode(f_name_ascii), float(max_memory_in_Gbytes), int(selected_locus),
                                     _dims(dims), out.ctypes.data_as(C.POINTER(C.c_int))))
    return out


def last_scan_argmax(device=0):
    """find_qtl.R:71-83 evaluated on the device on the last scan: (1-based index, tsq max, near ties)."""
    L = _lib.load()
    ctx = context(device)
    idx = C.c_long()
    mx = C.c_double()
    ties = C.c_long()
    _check(ctx, L.eagle_last_scan_argmax(ctx, C.byref(idx), C.byref(mx), C.byref(ties)))
    return idx.value, mx.value, ties.value


class _StreamStats(C.Structure):
    _fields_ = [("chunks", C.c_long), ("file_bytes", C.c_long), ("pread_s", C.c_double), ("load_s", C.c_double),
                ("wait_s", C.c_double), ("kernel_s", C.c_double), ("wall_s", C.c_double), ("load_first_s", C.c_double),
                ("starved_s", C.c_double)]


def last_stream_stats(device=0):
    """Out-of-core bookkeeping of the last call that streamed its file in marker chunks (include/eagle_hip.h,
    eagle_last_stream_stats), plus the derived storage rate and the fraction of the load time hidden under kernels."""
    L = _lib.load()
    ctx = context(device)
    st = _StreamStats()
    _check(ctx, L.eagle_last_stream_stats(ctx, C.byref(st)))
    d = {k: getattr(st, k) for k, _ in _StreamStats._fields_}
    d["read_GBps"] = d["file_bytes"] / 1e9 / d["pread_s"] if d["pread_s"] > 0 else 0.0
    later = d["load_s"] - d["load_first_s"]
    d["load_hidden_frac"] = max(0.0, 1.0 - d["starved_s"] / later) if later > 0 else 1.0
    return d


def last_scan_certificate(device=0):
    """(markers re-evaluated in fp64, of which flagged by their own error bound, whether a block fell back to fp64 entirely) of the
    last digit-slice calculate_a_and_vara_rcpp call (include/eagle_hip.h, eagle_last_scan_certificate)."""
    L = _lib.load()
    ctx = context(device)
    nre, nfl, fell = C.c_long(), C.c_long(), C.c_int()
    _check(ctx, L.eagle_last_scan_certificate(ctx, C.byref(nre), C.byref(nfl), C.byref(fell)))
    return nre.value, nfl.value, bool(fell.value)


def last_scan_digits(device=0):
    """(digit slices the last digit-slice scan used, slices cut from W, spectral bound or 0.0): eagle_last_scan_digits."""
    L = _lib.load()
    ctx = context(device)
    used, cut, H = C.c_int(), C.c_int(), C.c_double()
    _check(ctx, L.eagle_last_scan_digits(ctx, C.byref(used), C.byref(cut), C.byref(H)))
    return used.value, cut.value, H.value


class _ScanTiming(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("call_wall_s", "device_wall_s", "host_setup_s", "upload_ms", "w_ms", "load_wait_ms", "prepare_ms",
                                          "vara_ms", "certify_ms", "d2h_ms")] + [("blocks", C.c_long), ("markers", C.c_long)]


def last_scan_timing(device=0, device_index=0):
    """Phase clock of the last calculate_a_and_vara_rcpp / scan_with_W call on one device of the context (include/eagle_hip.h,
    eagle_last_scan_timing)."""
    L = _lib.load()
    ctx = context(device)
    st = _ScanTiming()
    _check(ctx, L.eagle_last_scan_timing(ctx, int(device_index), C.byref(st)))
    return {k: getattr(st, k) for k, _ in _ScanTiming._fields_}


def scan_operand_cache_stats(device=0):
    """(hits, misses) of the device copy of S = inv_MMt_sqrt kept between calculate_a_and_vara_rcpp calls (include/eagle_hip.h)."""
    L = _lib.load()
    ctx = context(device)
    h, m = C.c_long(), C.c_long()
    _check(ctx, L.eagle_scan_operand_cache_stats(ctx, C.byref(h), C.byref(m)))
    return h.value, m.value


def w8_keep_stats(device=0):
    """(hits, misses): calls of the int8 W engine that found what it keeps with S (digit image, row statistics, S 1) in place / had to
    compute it, summed over the devices of the context (eagle_w8_keep_stats, include/eagle_hip.h)."""
    L = _lib.load()
    ctx = context(device)
    h, m = C.c_long(), C.c_long()
    _check(ctx, L.eagle_w8_keep_stats(ctx, C.byref(h), C.byref(m)))
    return h.value, m.value


def last_mmt_normalised(n, device=0):
    """calcMMt.R:13 applied on the device to the last calculateMMt result."""
    L = _lib.load()
    ctx = context(device)
    out = np.zeros((n, n), dtype=np.float64, order="F")
    mx = C.c_double()
    _check(ctx, L.eagle_last_mmt_normalised(ctx, _dp(out), C.byref(mx)))
    return out, mx.value


# ---- marker-file ingestion (E/src/RcppExports.cpp:92-151): same argument order as the reference's exports ----
def getRowColumn(fname, device=0):
    L = _lib.load()
    ctx = context(device)
    d = (C.c_long * 2)()
    _check(ctx, L.eagle_get_row_column(ctx, os.fsencode(fname), d))
    return [int(d[0]), int(d[1])]


RESHAPE_FILES, RESHAPE_VIEW = 0, 1
_views = {}   # device -> alias paths registered by ReshapeM_rcpp(view=True)


def ReshapeM_rcpp(fnameM, fnameMt, indxNA, dims, view=False, device=0):
    """-> newdims (ReshapeM_rcpp.cpp:17-120): the individuals indxNA (0-based, any order) dropped from M.ascii and Mt.ascii
    under the names fnameM + "tmp" / fnameMt + "tmp".  view=False writes both files (host I/O only: no device is opened) and,
    when `device`'s context is open, drops views of the same names from it so that its later calls read the new files;
    view=True writes nothing and registers the two names as views on this device's context, which every later call of this
    module with the same `device` reads through (include/eagle_hip.h, eagle_reshape_m)."""
    L = _lib.load()
    na = np.ascontiguousarray(np.atleast_1d(np.asarray(indxNA, dtype=np.int64)).ravel(), dtype=np.int64)
    if na.size and not np.all(np.asarray(indxNA) == na):
        raise ValueError("ReshapeM_rcpp: indxNA must be whole numbers")
    out = (C.c_long * 2)()
    ctx = context(device) if view else _ctx.get(device)   # FILES: an open context forgets its views of these names
    rc = L.eagle_reshape_m(ctx, os.fsencode(fnameM), os.fsencode(fnameMt), na.ctypes.data_as(c_lp), na.size, _dims(dims),
                           RESHAPE_VIEW if view else RESHAPE_FILES, out)
    if rc != 0:
        raise EagleError(rc, L.eagle_last_error(ctx).decode())
    names = _views.setdefault(device, set())
    for f in (str(fnameM) + "tmp", str(fnameMt) + "tmp"):
        (names.add if view else names.discard)(f)
    return [int(out[0]), int(out[1])]


def view_load_counts(device=0):
    """Windows of view aliases loaded so far on `device`'s context, by source (eagle_view_load_counts)."""
    L = _lib.load()
    ctx = context(device)
    out = (C.c_long * 4)()
    _check(ctx, L.eagle_view_load_counts(ctx, out))
    return dict(zip(("resident", "sidecar", "text", "scanner"), (int(v) for v in out)))


def is_view(path, device=0):
    """True when `path` is a view alias registered on `device`'s context (no file of that name need exist)."""
    return str(path) in _views.get(device, ())


def createM_ASCII_rcpp(f_name, f_name_ascii, type, AA, AB, BB, max_memory_in_Gbytes, dims, quiet=True, message=None,
                       missing="NA", device=0):
    """-> bool it_worked (createM_ASCII_rcpp.cpp:18-106).  last_error() describes a False."""
    L = _lib.load()
    ctx = context(device)
    _set_message(ctx, message)
    enc = lambda v: str(v).encode()  # R passes AA=0, AB=1, BB=2 through as.character
    rc = _check(ctx, L.eagle_create_M_ascii(ctx, os.fsencode(f_name), os.fsencode(f_name_ascii), enc(type), enc(AA), enc(AB),
                                            enc(BB), float(max_memory_in_Gbytes), _dims(dims), int(bool(quiet)), enc(missing)),
                soft_ok=True)
    return rc == 0


def createMt_ASCII_rcpp(f_name, f_name_ascii, type, max_memory_in_Gbytes, dims, quiet=True, message=None, device=0):
    L = _lib.load()
    ctx = context(device)
    _set_message(ctx, message)
    _check(ctx, L.eagle_create_Mt_ascii(ctx, os.fsencode(f_name), os.fsencode(f_name_ascii), str(type).encode(),
                                        float(max_memory_in_Gbytes), _dims(dims), int(bool(quiet))))


def create_ascii_from_bed(bed_path, f_name_ascii_M, f_name_ascii_Mt, max_memory_in_Gbytes, dims, quiet=True, message=None, device=0):
    """-> number of missing genotypes (coded as heterozygotes).  M.ascii and Mt.ascii, their sidecars and resident images from a
    SNP-major PLINK .bed file of dims = (n individuals, L markers): eagle_create_ascii_from_bed (include/eagle_hip.h section 1b)."""
    L = _lib.load()
    ctx = context(device)
    _set_message(ctx, message)
    n_missing = C.c_long(0)
    _check(ctx, L.eagle_create_ascii_from_bed(ctx, os.fsencode(bed_path), os.fsencode(f_name_ascii_M), os.fsencode(f_name_ascii_Mt),
                                              float(max_memory_in_Gbytes), _dims(dims), int(bool(quiet)), C.byref(n_missing)))
    return int(n_missing.value)


# ---- marker QC (include/eagle_hip.h section 1b'): integer counts and filtered panels; the statistics are r_api's ----
def marker_counts(f_name_ascii_Mt, dims, max_memory_in_Gbytes=8.0, device=0):
    """eagle_marker_counts -> int32 (L, 3): the numbers of '0', '1', '2' characters of every line of Mt.ascii (dims = (n, L) of M).
    A view alias gives the counts over its kept individuals."""
    L = _lib.load()
    ctx = context(device)
    out = np.zeros((int(dims[1]), 3), dtype=np.int32)
    _check(ctx, L.eagle_marker_counts(ctx, os.fsencode(f_name_ascii_Mt), _dims(dims), float(max_memory_in_Gbytes),
                                      out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


def bed_marker_counts(bed_path, dims, max_memory_in_Gbytes=8.0, device=0):
    """eagle_bed_marker_counts -> int32 (L, 4): homozygous A1, heterozygous, homozygous A2, missing of every marker of a SNP-major
    PLINK .bed file of dims = (n individuals, L markers)."""
    L = _lib.load()
    ctx = context(device)
    out = np.zeros((int(dims[1]), 4), dtype=np.int32)
    _check(ctx, L.eagle_bed_marker_counts(ctx, os.fsencode(bed_path), _dims(dims), float(max_memory_in_Gbytes),
                                          out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


VCF_A2_ALT, VCF_SNPS_ONLY, VCF_PASS_ONLY = 1, 2, 4      # the flags of include/eagle_hip.h section 1b-vcf
VCF_COUNT_FIELDS = tuple(f for f, _ in _lib.VcfCounts._fields_)


def vcf_flags(a2="ref", snps_only=False, pass_only=False):
    """The flag word of eagle_vcf_to_bed: a2 = "ref" (A1 = ALT, A2 = REF, the default) or "alt" (A2 = ALT)."""
    if a2 not in ("ref", "alt"):
        raise ValueError('vcf_to_bed: a2 must be "ref" or "alt"')
    return (VCF_A2_ALT if a2 == "alt" else 0) | (VCF_SNPS_ONLY if snps_only else 0) | (VCF_PASS_ONLY if pass_only else 0)


def vcf_to_bed(vcf, out_prefix, a2="ref", snps_only=False, pass_only=False, availmemGb=8, chunk_bytes=0, device=0):
    """eagle_vcf_to_bed -> {"bed", "bim", "fam", "dims", "counts"}: the plain-text VCF file `vcf` as the PLINK binary fileset
    out_prefix + ".bed" / ".bim" / ".fam", its GT fields decoded on the device.  dims = [n samples, kept markers]; counts = the
    eagle_vcf_counts of the call as a dict.  chunk_bytes caps the text staged per window (0: from availmemGb); the files do not depend
    on it.  The arguments are checked by the library before it needs a device: EagleError(-3, ...) then, without opening one."""
    L = _lib.load()
    flags = vcf_flags(a2, snps_only, pass_only)
    dims, counts = (C.c_long * 2)(), _lib.VcfCounts()
    prefix = os.fspath(out_prefix)
    _args_first(L.eagle_vcf_to_bed, device, (os.fsencode(vcf), os.fsencode(prefix), flags, float(availmemGb), int(chunk_bytes), dims,
                                             C.byref(counts)))
    return {"bed": prefix + ".bed", "bim": prefix + ".bim", "fam": prefix + ".fam", "dims": [int(dims[0]), int(dims[1])],
            "counts": {f: int(getattr(counts, f)) for f in VCF_COUNT_FIELDS}}


def filter_markers(fnameM, fnameMt, dims, keep, outM, outMt, max_memory_in_Gbytes=8.0, device=0):
    """eagle_filter_markers -> newdims [n, nkeep]: outM / outMt, their sidecars and resident images for the markers `keep` (0-based,
    strictly increasing) of the panel (fnameM, fnameMt; dims = (n, L) of M).  The keep-list and the paths are checked by the library
    before it needs a device: EagleError(-3, ...) then, without opening one."""
    L = _lib.load()
    kv = np.ascontiguousarray(np.atleast_1d(np.asarray(keep, dtype=np.int64)).ravel(), dtype=np.int64)
    if kv.size and not np.all(np.asarray(keep).ravel() == kv):
        raise ValueError("filter_markers: keep must hold whole numbers")
    out = (C.c_long * 2)()
    args = (os.fsencode(fnameM), os.fsencode(fnameMt), _dims(dims), kv.ctypes.data_as(c_lp), kv.size, os.fsencode(outM), os.fsencode(outMt),
            float(max_memory_in_Gbytes), out)
    if device not in _ctx:   # argument errors first: they need no context (text through eagle_open_error)
        if L.eagle_filter_markers(None, *args) == -3 and b"no context" not in L.eagle_open_error():
            raise EagleError(-3, L.eagle_open_error().decode())
    ctx = context(device)
    _check(ctx, L.eagle_filter_markers(ctx, *args))
    return [int(out[0]), int(out[1])]


# ---- linkage disequilibrium (include/eagle_hip.h section 1b''): integer masks and dot products; r^2 and the pruning are r_api's ----
def _args_first(fn, device, args):
    """Argument errors need no context (their text comes through eagle_open_error): a bad call does not open a device."""
    L = _lib.load()
    if device not in _ctx:
        if fn(None, *args) == -3 and b"no context" not in L.eagle_open_error():
            raise EagleError(-3, L.eagle_open_error().decode())
    ctx = context(device)
    _check(ctx, fn(ctx, *args))


def ld_window(f_name_ascii_Mt, dims, window=50, r2=0.2, max_memory_in_Gbytes=8.0, device=0, return_pairs=False):
    """eagle_ld_window -> uint64 (L, ceil(window / 64)): bit (o - 1) % 64 of word (o - 1) // 64 of row i is set iff markers i and
    i + o, 1 <= o <= window, are in LD at r2 (the rule of include/eagle_hip.h section 1b'').  return_pairs: (mask, number of set bits)."""
    L = _lib.load()
    out = np.zeros((int(dims[1]), (int(window) + 63) // 64 if int(window) > 0 else 1), dtype=np.uint64)
    pairs = C.c_long(0)
    _args_first(L.eagle_ld_window, device, (os.fsencode(f_name_ascii_Mt), _dims(dims), int(window), float(r2), float(max_memory_in_Gbytes),
                                            out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(pairs)))
    return (out, int(pairs.value)) if return_pairs else out


def ld_dots(f_name_ascii_Mt, dims, loci, max_memory_in_Gbytes=8.0, device=0):
    """eagle_ld_dots -> int32 (L, k): the sum over the individuals of g_i g_j for every marker i and the k <= 64 markers j = loci
    (0-based, repeats allowed)."""
    L = _lib.load()
    lv = np.ascontiguousarray(np.atleast_1d(np.asarray(loci, dtype=np.int64)).ravel(), dtype=np.int64)
    if lv.size and not np.all(np.asarray(loci).ravel() == lv):
        raise ValueError("ld_dots: loci must hold whole numbers")
    out = np.zeros((int(dims[1]), max(int(lv.size), 1)), dtype=np.int32)
    _args_first(L.eagle_ld_dots, device, (os.fsencode(f_name_ascii_Mt), _dims(dims), lv.ctypes.data_as(c_lp), lv.size, float(max_memory_in_Gbytes),
                                          out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


# ---- sample QC (include/eagle_hip.h section 1b'''): integer counts and exact-test p-values; kinship and the filters are r_api's ----
_c_i32p = C.POINTER(C.c_int32)


def sample_counts(f_name_ascii_M, dims, max_memory_in_Gbytes=8.0, device=0):
    """eagle_sample_counts -> int32 (n, 3): the numbers of '0', '1', '2' characters of every line of M.ascii (dims = (n, L) of M), the
    genotype counts of every individual.  A view alias gives the counts of its kept individuals."""
    L = _lib.load()
    out = np.zeros((int(dims[0]), 3), dtype=np.int32)
    _args_first(L.eagle_sample_counts, device, (os.fsencode(f_name_ascii_M), _dims(dims), float(max_memory_in_Gbytes), out.ctypes.data_as(_c_i32p)))
    return out


def bed_sample_counts(bed_path, dims, max_memory_in_Gbytes=8.0, device=0):
    """eagle_bed_sample_counts -> int32 (n, 4): homozygous A1, heterozygous, homozygous A2, missing of every individual of a SNP-major
    PLINK .bed file of dims = (n individuals, L markers)."""
    L = _lib.load()
    out = np.zeros((int(dims[0]), 4), dtype=np.int32)
    _args_first(L.eagle_bed_sample_counts, device, (os.fsencode(bed_path), _dims(dims), float(max_memory_in_Gbytes), out.ctypes.data_as(_c_i32p)))
    return out


def sample_ibs(f_name_ascii_M, dims, max_memory_in_Gbytes=8.0, device=0):
    """eagle_sample_ibs -> (ibs0, hethet), int32 (n, n) each: for every pair of individuals the markers where they are opposite
    homozygotes and the markers where both are heterozygous (diagonal: 0 and the individual's heterozygous genotypes)."""
    L = _lib.load()
    n = int(dims[0])
    ibs0, hethet = np.zeros((n, n), dtype=np.int32), np.zeros((n, n), dtype=np.int32)
    _args_first(L.eagle_sample_ibs, device, (os.fsencode(f_name_ascii_M), _dims(dims), float(max_memory_in_Gbytes), ibs0.ctypes.data_as(_c_i32p),
                                             hethet.ctypes.data_as(_c_i32p)))
    return ibs0, hethet


def hwe_exact(counts, device=0):
    """eagle_hwe_exact -> fp64 (L): the Hardy-Weinberg exact test of counts = int (L, 3) or (L, 4) rows (n_AA, n_AB, n_BB[, unused]):
    what marker_counts and bed_marker_counts return."""
    L = _lib.load()
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[1] not in (3, 4):
        raise ValueError("hwe_exact: counts must be (L, 3) or (L, 4)")
    c32 = np.ascontiguousarray(c, dtype=np.int32)
    if not np.array_equal(c32, c):
        raise ValueError("hwe_exact: counts must hold whole numbers that fit int32")
    out = np.zeros(c32.shape[0], dtype=np.float64)
    _args_first(L.eagle_hwe_exact, device, (c32.ctypes.data_as(_c_i32p), c32.shape[0], c32.shape[1], _dp(out)))
    return out


# ---- kNN imputation (include/eagle_hip.h section 1b'''i): the neighbour table and the patched .bed file; r_api holds the restatements ----
def _i32_matrix(a, what):
    m = np.asarray(a)
    m32 = np.ascontiguousarray(m, dtype=np.int32)
    if m32.ndim != 2 or not np.array_equal(m32, m):
        raise ValueError("%s must be a matrix of whole numbers that fit int32" % what)
    return m32


def knn_rows(ibs0, hethet, K, device=0):
    """eagle_knn_rows -> int32 (n, K): row i = the min(K, n - 1) individuals j != i with the smallest distance
    d_ij = 4 ibs0_ij + h_i + h_j - 2 hethet_ij (h = diag(hethet)), nearest first, ties to the smaller index; -1 beyond them.
    ibs0, hethet: the (n, n) matrices of sample_ibs."""
    L = _lib.load()
    a, h = _i32_matrix(ibs0, "knn_rows: ibs0"), _i32_matrix(hethet, "knn_rows: hethet")
    if a.shape[0] != a.shape[1] or a.shape != h.shape:
        raise ValueError("knn_rows: ibs0 and hethet must be square and of one shape")
    out = np.zeros((a.shape[0], max(int(K), 1)), dtype=np.int32)
    _args_first(L.eagle_knn_rows, device, (a.ctypes.data_as(_c_i32p), h.ctypes.data_as(_c_i32p), a.shape[0], int(K), out.ctypes.data_as(_c_i32p)))
    return out


DIST_NO_OVERLAP = 0xFFFFFFFE    # bed_sample_ibs' dist of a pair with fewer than min_overlap markers where both are called


def bed_sample_ibs(bed_path, dims, include=None, min_overlap=1, max_memory_in_Gbytes=8.0, device=0):
    """eagle_bed_sample_ibs -> (ncalled, ibs0, hethet, hetsum, dist): int32 (n, n) x 4 and uint32 (n, n), the pairwise-complete counts
    of include/eagle_hip.h section 1b'''ii from a SNP-major PLINK .bed file of dims = (n individuals, L markers) -- for every pair the
    markers where both are called, where they are opposite homozygotes, where both are heterozygous, the heterozygous genotypes of
    either where the other is called -- and the distance sum (g_i - g_j)^2 over the both-called markers scaled to the included markers
    (DIST_NO_OVERLAP below min_overlap).  include: None, or a bool / 0-1 mask of length L; r_api.bed_ibs_host is the numpy restatement."""
    L = _lib.load()
    n, nm = int(dims[0]), int(dims[1])
    inc = None
    if include is not None:
        inc = np.ascontiguousarray(np.atleast_1d(np.asarray(include)).ravel() != 0, dtype=np.uint8)
        if inc.size != nm:
            raise ValueError("bed_sample_ibs: include holds %d entries, the file %d markers" % (inc.size, nm))
    out = [np.zeros((max(n, 0), max(n, 0)), dtype=np.int32) for _ in range(4)]
    dist = np.zeros((max(n, 0), max(n, 0)), dtype=np.uint32)
    _args_first(L.eagle_bed_sample_ibs, device, (os.fsencode(bed_path), _dims(dims), inc.ctypes.data_as(C.c_void_p) if inc is not None else None,
                                                 int(min_overlap), float(max_memory_in_Gbytes), out[0].ctypes.data_as(_c_i32p),
                                                 out[1].ctypes.data_as(_c_i32p), out[2].ctypes.data_as(_c_i32p), out[3].ctypes.data_as(_c_i32p),
                                                 dist.ctypes.data_as(C.c_void_p)))
    return out[0], out[1], out[2], out[3], dist


def knn_rows_dist(dist, K, device=0):
    """eagle_knn_rows_dist -> int32 (n, K): row i = the min(K, n - 1) individuals j != i with the smallest dist_ij, nearest first, ties
    to the smaller index; -1 beyond them.  dist: the uint32 (n, n) matrix of bed_sample_ibs."""
    L = _lib.load()
    m = np.asarray(dist)
    d = np.ascontiguousarray(m, dtype=np.uint32)
    if d.ndim != 2 or d.shape[0] != d.shape[1] or not np.array_equal(d, m):
        raise ValueError("knn_rows_dist: dist must be a square matrix of whole numbers that fit uint32")
    out = np.zeros((d.shape[0], max(int(K), 1)), dtype=np.int32)
    _args_first(L.eagle_knn_rows_dist, device, (d.ctypes.data_as(C.c_void_p), d.shape[0], int(K), out.ctypes.data_as(_c_i32p)))
    return out


def bed_impute_knn(bed_path, dims, nbr, k, min_votes, out_bed_path, max_memory_in_Gbytes=8.0, device=0):
    """eagle_bed_impute_knn -> int32 (L, 2): the genotypes of every marker imputed by vote and by fallback.  Writes out_bed_path, the
    SNP-major .bed file bed_path (dims = (n individuals, L markers)) with every missing genotype filled from the first k called
    neighbours of nbr ((n, K) int32: knn_rows), or from the marker's own calls when fewer than min_votes of them are called."""
    L = _lib.load()
    nb = _i32_matrix(nbr, "bed_impute_knn: nbr")
    if nb.shape[0] != int(dims[0]):
        raise ValueError("bed_impute_knn: nbr holds %d rows, the file %d individuals" % (nb.shape[0], int(dims[0])))
    out = np.zeros((max(int(dims[1]), 0), 2), dtype=np.int32)
    _args_first(L.eagle_bed_impute_knn, device, (os.fsencode(bed_path), _dims(dims), nb.ctypes.data_as(_c_i32p), nb.shape[1], int(k), int(min_votes),
                                                 os.fsencode(out_bed_path), float(max_memory_in_Gbytes), out.ctypes.data_as(_c_i32p)))
    return out


# ---- LD-kNNi (include/eagle_hip.h section 1b'''iii): ranked LD partners per marker and the .bed file patched from them ----
LDKNN_MAX_PARTNERS = 32
LDKNN_MAX_K = 64
LDKNN_MAX_N = 12288


def ld_partners(f_name_ascii_Mt, dims, window=50, l=16, min_r2=0.0, chrom=None, max_memory_in_Gbytes=8.0, device=0, return_r2=False):
    """eagle_ld_partners -> int32 (L, l): row i = the markers j, 1 <= |j - i| <= window, on i's chromosome when chrom (L whole numbers)
    is given, with r2_ij >= min_r2, by decreasing r2 (ties to the smaller |j - i|, then the smaller j); -1 beyond them.  r2 is the fp64
    number of include/eagle_hip.h section 1b'''iii.  return_r2: (partners, fp64 (L, l) with 0.0 beside -1).  r_api.ld_partners_host is
    the numpy restatement."""
    L = _lib.load()
    nm = max(int(dims[1]), 0)
    ch = None
    if chrom is not None:
        c = np.atleast_1d(np.asarray(chrom)).ravel()
        ch = np.ascontiguousarray(c, dtype=np.int32)
        if ch.size != nm or not np.array_equal(ch, c):
            raise ValueError("ld_partners: chrom must hold one whole number that fits int32 per marker")
    out = np.zeros((nm, max(int(l), 1)), dtype=np.int32)
    r2 = np.zeros(out.shape, dtype=np.float64) if return_r2 else None
    _args_first(L.eagle_ld_partners, device, (os.fsencode(f_name_ascii_Mt), _dims(dims), int(window), int(l), float(min_r2),
                                              ch.ctypes.data_as(_c_i32p) if ch is not None else None, float(max_memory_in_Gbytes),
                                              out.ctypes.data_as(_c_i32p), _dp(r2) if return_r2 else None))
    return (out, r2) if return_r2 else out


def bed_impute_ldknn(bed_path, dims, partners, k, min_votes, min_overlap, out_bed_path, max_memory_in_Gbytes=8.0, device=0):
    """eagle_bed_impute_ldknn -> int32 (L, 2): the genotypes of every marker imputed by vote and by fallback.  Writes out_bed_path, the
    SNP-major .bed file bed_path (dims = (n individuals, L markers)) with every missing genotype filled from the k individuals that
    are called at its marker and nearest over the marker's partners ((L, l) int32: ld_partners), among those compared over at least
    min_overlap partners; from the marker's own calls when fewer than min_votes of them exist."""
    L = _lib.load()
    pt = _i32_matrix(partners, "bed_impute_ldknn: partners")
    if pt.shape[0] != int(dims[1]):
        raise ValueError("bed_impute_ldknn: partners holds %d rows, the file %d markers" % (pt.shape[0], int(dims[1])))
    out = np.zeros((max(int(dims[1]), 0), 2), dtype=np.int32)
    _args_first(L.eagle_bed_impute_ldknn, device, (os.fsencode(bed_path), _dims(dims), pt.ctypes.data_as(_c_i32p), pt.shape[1], int(k), int(min_votes),
                                                   int(min_overlap), os.fsencode(out_bed_path), float(max_memory_in_Gbytes),
                                                   out.ctypes.data_as(_c_i32p)))
    return out


# ---- pairwise-complete LD from the .bed file (include/eagle_hip.h section 1b'''iv): ld_window / ld_partners over the both-called individuals ----
def _bed_ld_include(include, nm, who):
    if include is None:
        return None
    inc = np.ascontiguousarray(np.atleast_1d(np.asarray(include)).ravel() != 0, dtype=np.uint8)
    if inc.size != nm:
        raise ValueError("%s: include holds %d entries, the file %d markers" % (who, inc.size, nm))
    return inc


def bed_ld_window(bed_path, dims, window=50, r2=0.2, include=None, min_overlap=1, availmemGb=8.0, device=0, return_pairs=False):
    """eagle_bed_ld_window -> uint64 (Linc, ceil(window / 64)): ld_window's mask from a SNP-major PLINK .bed file of dims = (n individuals,
    L markers), every pair of markers counted over the individuals called at both (at least min_overlap of them; the rule of
    include/eagle_hip.h section 1b'''iv).  include: None, or a bool / 0-1 mask of length L that selects the panel; rows and offsets are
    panel indices.  return_pairs: (mask, number of set bits).  r_api.bed_ld_mask_host is the numpy restatement."""
    L = _lib.load()
    nm = max(int(dims[1]), 0)
    inc = _bed_ld_include(include, nm, "bed_ld_window")
    linc = nm if inc is None else int(inc.sum())
    out = np.zeros((linc, (int(window) + 63) // 64 if int(window) > 0 else 1), dtype=np.uint64)
    pairs = C.c_long(0)
    _args_first(L.eagle_bed_ld_window, device, (os.fsencode(bed_path), _dims(dims), inc.ctypes.data_as(C.c_void_p) if inc is not None else None,
                                                int(window), float(r2), int(min_overlap), float(availmemGb),
                                                out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(pairs)))
    return (out, int(pairs.value)) if return_pairs else out


def bed_ld_partners(bed_path, dims, window=50, l=16, min_r2=0.0, include=None, min_overlap=1, chrom=None, availmemGb=8.0, device=0,
                    return_r2=False):
    """eagle_bed_ld_partners -> int32 (Linc, l): ld_partners' table from a SNP-major PLINK .bed file, r2 of every pair over the individuals
    called at both markers (at least min_overlap of them, and both markers polymorphic over them; include/eagle_hip.h section 1b'''iv).
    include as in bed_ld_window; chrom: one whole number per PANEL marker.  return_r2: (partners, fp64 (Linc, l) with 0.0 beside -1).
    r_api.bed_ld_partners_host is the numpy restatement."""
    L = _lib.load()
    nm = max(int(dims[1]), 0)
    inc = _bed_ld_include(include, nm, "bed_ld_partners")
    linc = nm if inc is None else int(inc.sum())
    ch = None
    if chrom is not None:
        c = np.atleast_1d(np.asarray(chrom)).ravel()
        ch = np.ascontiguousarray(c, dtype=np.int32)
        if ch.size != linc or not np.array_equal(ch, c):
            raise ValueError("bed_ld_partners: chrom must hold one whole number that fits int32 per panel marker")
    out = np.zeros((linc, max(int(l), 1)), dtype=np.int32)
    r2 = np.zeros(out.shape, dtype=np.float64) if return_r2 else None
    _args_first(L.eagle_bed_ld_partners, device, (os.fsencode(bed_path), _dims(dims), inc.ctypes.data_as(C.c_void_p) if inc is not None else None,
                                                  int(window), int(l), float(min_r2), int(min_overlap),
                                                  ch.ctypes.data_as(_c_i32p) if ch is not None else None, float(availmemGb),
                                                  out.ctypes.data_as(_c_i32p), _dp(r2) if return_r2 else None))
    return (out, r2) if return_r2 else out


# ---- LD scores and the LD decay curve (include/eagle_hip.h section 1b'''v): the r2 band summed as exact integers ----
LD_STATS_MAX_BINS = 512
_c_i64p = C.POINTER(C.c_int64)
_c_u64p = C.POINTER(C.c_uint64)


def _ld_stats_args(who, nm, chrom, pos, max_dist, edges):
    """The per-marker arrays and the bin edges of an ld_stats call as the C side takes them; ValueError before the library is called."""
    ch = ps = ed = None
    if chrom is not None:
        c = np.atleast_1d(np.asarray(chrom)).ravel()
        ch = np.ascontiguousarray(c, dtype=np.int32)
        if ch.size != nm or not np.array_equal(ch, c):
            raise ValueError("%s: chrom must hold one whole number that fits int32 per panel marker" % who)
    if pos is not None:
        c = np.atleast_1d(np.asarray(pos)).ravel()
        ps = np.ascontiguousarray(c, dtype=np.int64)
        if ps.size != nm or not np.array_equal(ps, c):
            raise ValueError("%s: pos must hold one whole number of base pairs per panel marker" % who)
    if int(max_dist) > 0 and ps is None:
        raise ValueError("%s: max_dist needs pos" % who)
    if edges is not None:
        c = np.atleast_1d(np.asarray(edges)).ravel()
        ed = np.ascontiguousarray(c, dtype=np.int64)
        if not 2 <= ed.size <= LD_STATS_MAX_BINS + 1 or not np.array_equal(ed, c) or np.any(np.diff(ed) <= 0):
            raise ValueError("%s: edges must be 2 to %d strictly increasing whole numbers" % (who, LD_STATS_MAX_BINS + 1))
    return ch, ps, ed


def ld_stats(f_name_ascii_Mt, dims, window=50, chrom=None, pos=None, max_dist=0, edges=None, max_memory_in_Gbytes=8.0, device=0):
    """eagle_ld_stats -> (U uint64 (L), cnt int32 (L)), with edges also (bin_sum uint64 (B), bin_pairs int64 (B)), B = len(edges) - 1:
    the sums of include/eagle_hip.h section 1b'''v over the r2 band of the ingested panel.  U_i = the sum of u_ij = (uint64)(r2_ij * 2^30)
    over the markers j with 1 <= |j - i| <= window, r2_ij >= 0, chrom[j] == chrom[i] (chrom: L whole numbers) and |pos[j] - pos[i]| <=
    max_dist (pos: L whole numbers of base pairs, max_dist > 0); cnt_i their number; the LD score is 1 + U / 2^30.  Every such pair
    i < j adds u_ij and 1 to the bin b with edges[b] <= d_ij < edges[b + 1], d = |pos[j] - pos[i]| with pos and j - i without.
    r_api.ld_stats_host(r_api.ld_band_host(Mt8, window), ...) is the numpy restatement."""
    L = _lib.load()
    nm = max(int(dims[1]), 0)
    ch, ps, ed = _ld_stats_args("ld_stats", nm, chrom, pos, max_dist, edges)
    nb = 0 if ed is None else ed.size - 1
    U, cnt = np.zeros(nm, dtype=np.uint64), np.zeros(nm, dtype=np.int32)
    bsum, bpairs = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.int64)
    _args_first(L.eagle_ld_stats, device, (os.fsencode(f_name_ascii_Mt), _dims(dims), int(window),
                                           ch.ctypes.data_as(_c_i32p) if ch is not None else None,
                                           ps.ctypes.data_as(_c_i64p) if ps is not None else None, int(max_dist),
                                           ed.ctypes.data_as(_c_i64p) if ed is not None else None, nb, float(max_memory_in_Gbytes),
                                           U.ctypes.data_as(_c_u64p), cnt.ctypes.data_as(_c_i32p),
                                           bsum.ctypes.data_as(_c_u64p) if nb else None, bpairs.ctypes.data_as(_c_i64p) if nb else None))
    return (U, cnt, bsum, bpairs) if nb else (U, cnt)


def bed_ld_stats(bed_path, dims, window=50, include=None, min_overlap=1, chrom=None, pos=None, max_dist=0, edges=None, availmemGb=8.0,
                 device=0):
    """eagle_bed_ld_stats -> ld_stats' tuple by PANEL marker from a SNP-major PLINK .bed file, r2 of every pair over the individuals
    called at both markers (at least min_overlap of them; include/eagle_hip.h section 1b'''iv).  include as in bed_ld_window; chrom and
    pos: one whole number per panel marker.  r_api.ld_stats_host(r_api.bed_ld_host(...)[6], ...) is the numpy restatement."""
    L = _lib.load()
    nm = max(int(dims[1]), 0)
    inc = _bed_ld_include(include, nm, "bed_ld_stats")
    linc = nm if inc is None else int(inc.sum())
    ch, ps, ed = _ld_stats_args("bed_ld_stats", linc, chrom, pos, max_dist, edges)
    nb = 0 if ed is None else ed.size - 1
    U, cnt = np.zeros(linc, dtype=np.uint64), np.zeros(linc, dtype=np.int32)
    bsum, bpairs = np.zeros(nb, dtype=np.uint64), np.zeros(nb, dtype=np.int64)
    _args_first(L.eagle_bed_ld_stats, device, (os.fsencode(bed_path), _dims(dims), inc.ctypes.data_as(C.c_void_p) if inc is not None else None,
                                               int(window), int(min_overlap), ch.ctypes.data_as(_c_i32p) if ch is not None else None,
                                               ps.ctypes.data_as(_c_i64p) if ps is not None else None, int(max_dist),
                                               ed.ctypes.data_as(_c_i64p) if ed is not None else None, nb, float(availmemGb),
                                               U.ctypes.data_as(_c_u64p), cnt.ctypes.data_as(_c_i32p),
                                               bsum.ctypes.data_as(_c_u64p) if nb else None, bpairs.ctypes.data_as(_c_i64p) if nb else None))
    return (U, cnt, bsum, bpairs) if nb else (U, cnt)


# ---- runs of homozygosity (include/eagle_hip.h section 1b'''vi): the window scan and the segment table as exact integers ----
ROH_MAX_WINDOW = 64
ROH_MAX_DENSITY = 1 << 31
ROH_DEFAULTS = dict(w=50, win_het=1, win_miss=5, thr16=3277, min_snp=100, min_len=0, max_gap=0, max_density=0, max_het=-1)
_ROH_FIELDS = ("w", "win_het", "win_miss", "thr16", "min_snp", "min_len", "max_gap", "max_density", "max_het")


def roh_params(who="roh", **params):
    """The nine integers of eagle_roh_params as a dict, defaults ROH_DEFAULTS; ValueError for an unknown name, a value that is not a whole
    number, or one outside the header's rule: w in [1, 64], thr16 in [0, 65536], min_snp >= 1, max_density in [0, 2^31], win_het,
    win_miss, min_len and max_gap >= 0 (max_het: any negative number switches the filter off)."""
    p = dict(ROH_DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise ValueError("%s: unknown parameter %s" % (who, k))
        try:
            iv = int(v)
        except (TypeError, ValueError):
            raise ValueError("%s: %s must be a whole number" % (who, k))
        if iv != v or not -(1 << 63) <= iv < 1 << 63:
            raise ValueError("%s: %s must be a whole number that fits int64" % (who, k))
        p[k] = iv
    if not 1 <= p["w"] <= ROH_MAX_WINDOW:
        raise ValueError("%s: w must be in [1, %d]" % (who, ROH_MAX_WINDOW))
    if not 0 <= p["thr16"] <= 65536:
        raise ValueError("%s: thr16 must be in [0, 65536]" % who)
    if p["min_snp"] < 1:
        raise ValueError("%s: min_snp must be at least 1" % who)
    if not 0 <= p["max_density"] <= ROH_MAX_DENSITY:
        raise ValueError("%s: max_density must be in [0, 2^31]" % who)
    for k in ("win_het", "win_miss", "min_len", "max_gap"):
        if p[k] < 0:
            raise ValueError("%s: %s must not be negative" % (who, k))
    return p


def roh_blocks(chrom, nm):
    """The block bounds of rule 2 -> int64 (nb + 1): 0 = blk[0] < ... < blk[nb] = nm, a block a maximal run of equal chrom."""
    if chrom is None or nm < 2:
        return np.array([0, nm], dtype=np.int64)
    c = np.asarray(chrom).ravel()
    return np.concatenate(([0], np.flatnonzero(c[1:] != c[:-1]) + 1, [nm])).astype(np.int64)


def _roh_args(who, nm, chrom, pos, params):
    ch, ps, _ = _ld_stats_args(who, nm, chrom, pos, 0, None)
    p = roh_params(who, **params)
    if nm >= 1 << 31:
        raise ValueError("%s: 2^31 markers or more" % who)
    if ps is not None:
        blk = roh_blocks(ch, nm)
        d = np.diff(ps) < 0
        d[blk[1:-1] - 1] = False                         # block edges are not compared across
        if d.any():
            raise ValueError("%s: pos decreases inside a block (panel marker %d)" % (who, int(np.flatnonzero(d)[0]) + 1))
    return ch, ps, _lib.RohParams(*[p[f] for f in _ROH_FIELDS])


def _roh_call(fn, device, head, ch, ps, prm, mem, n, seg_cap):
    ind = np.zeros((n, 4), dtype=np.int64)
    while True:
        seg = np.zeros((seg_cap, 6), dtype=np.int32)
        total = C.c_long(0)
        _args_first(fn, device, head + (ch.ctypes.data_as(_c_i32p) if ch is not None else None,
                                        ps.ctypes.data_as(_c_i64p) if ps is not None else None, C.addressof(prm), float(mem),
                                        ind.ctypes.data_as(_c_i64p), seg.ctypes.data_as(_c_i32p) if seg_cap else None, seg_cap, C.byref(total)))
        if total.value <= seg_cap:
            return ind, seg[:total.value].copy()
        seg_cap = int(total.value)


def roh(f_name_ascii_Mt, dims, chrom=None, pos=None, max_memory_in_Gbytes=8.0, device=0, seg_cap=None, **params):
    """eagle_roh -> (ind int64 (n, 4), seg int32 (S, 6)): the runs of homozygosity of include/eagle_hip.h section 1b'''vi on the ingested
    panel (dims = (n, L) of M).  ind = (segments, sum of nsnp, sum of len, longest len) per individual; seg rows = (individual, first
    marker, last marker, nhet, nmiss, block ordinal), sorted by (individual, first marker).  chrom, pos: one whole number per marker or
    None (one block; pos = the marker index).  params: w, win_het, win_miss, thr16, min_snp, min_len, max_gap, max_density, max_het
    (ROH_DEFAULTS).  The library is called once with a capacity guess (seg_cap, default 4 n) and once more if that was short.  ValueError
    for bad arguments before the library is called.  r_api.roh_host(r_api.roh_classes_mt8(Mt8), ...) is the numpy restatement."""
    L = _lib.load()
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    ch, ps, prm = _roh_args("roh", nm, chrom, pos, params)
    cap = 4 * n if seg_cap is None else int(seg_cap)
    if cap < 0:
        raise ValueError("roh: seg_cap must not be negative")
    return _roh_call(L.eagle_roh, device, (os.fsencode(f_name_ascii_Mt), _dims(dims)), ch, ps, prm, max_memory_in_Gbytes, n, cap)


def bed_roh(bed_path, dims, include=None, chrom=None, pos=None, availmemGb=8.0, device=0, seg_cap=None, **params):
    """eagle_bed_roh -> roh's pair by PANEL marker from a SNP-major PLINK .bed file of dims = (n individuals, L markers), which still
    knows its missing calls (code 01 is the class miss, counted against win_miss and in nmiss).  include as in bed_ld_window; chrom and
    pos: one whole number per panel marker.  r_api.roh_host(r_api.roh_classes_bed(read_bed_codes(...)[include]), ...) is the numpy
    restatement."""
    L = _lib.load()
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    inc = _bed_ld_include(include, nm, "bed_roh")
    linc = nm if inc is None else int(inc.sum())
    ch, ps, prm = _roh_args("bed_roh", linc, chrom, pos, params)
    cap = 4 * n if seg_cap is None else int(seg_cap)
    if cap < 0:
        raise ValueError("bed_roh: seg_cap must not be negative")
    head = (os.fsencode(bed_path), _dims(dims), inc.ctypes.data_as(C.c_void_p) if inc is not None else None)
    return _roh_call(L.eagle_bed_roh, device, head, ch, ps, prm, availmemGb, n, cap)


# ---- pairwise IBD-type segments (include/eagle_hip.h section 1b'''vii): shared-genotype runs between individuals as exact integers ----
IBD_MAX_PAIRS = 1 << 27
IBD_DEFAULTS = dict(mode=1, min_snp=200, min_len=0, max_gap=0, merge_min=100)
IBD_MODES = {"ibs1": 1, "ibs2": 2}
_IBD_FIELDS = ("mode", "min_snp", "min_len", "max_gap", "merge_min")


def ibd_params(who="ibd", **params):
    """The five integers of eagle_ibd_params as a dict, defaults IBD_DEFAULTS; mode may be "ibs1" / "ibs2".  ValueError for an unknown
    name, a value that is not a whole number, or one outside the header's rule: mode 1 or 2, min_snp >= 1, min_len, max_gap and
    merge_min >= 0."""
    p = dict(IBD_DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise ValueError("%s: unknown parameter %s" % (who, k))
        if k == "mode" and isinstance(v, str):
            if v not in IBD_MODES:
                raise ValueError("%s: mode must be 1 (ibs1) or 2 (ibs2)" % who)
            v = IBD_MODES[v]
        try:
            iv = int(v)
        except (TypeError, ValueError):
            raise ValueError("%s: %s must be a whole number" % (who, k))
        if iv != v or not -(1 << 63) <= iv < 1 << 63:
            raise ValueError("%s: %s must be a whole number that fits int64" % (who, k))
        p[k] = iv
    if p["mode"] not in (1, 2):
        raise ValueError("%s: mode must be 1 (ibs1) or 2 (ibs2)" % who)
    if p["min_snp"] < 1:
        raise ValueError("%s: min_snp must be at least 1" % who)
    for k in ("min_len", "max_gap", "merge_min"):
        if p[k] < 0:
            raise ValueError("%s: %s must not be negative" % (who, k))
    return p


def ibd_pairs(who, pairs, n):
    """A pair list as contiguous int32 (P, 2), or None for all pairs; ValueError for a pair outside 0 <= i < j < n or a count outside
    [1, 2^27] (all pairs: n >= 2 and n (n - 1) / 2 <= 2^27)."""
    if pairs is None:
        if n < 2:
            raise ValueError("%s: all pairs need at least two individuals" % who)
        if n * (n - 1) // 2 > IBD_MAX_PAIRS:
            raise ValueError("%s: more than 2^27 pairs: give a list" % who)
        return None
    a = np.asarray(pairs)
    if a.size == 0 or a.ndim != 2 or a.shape[1] != 2 or a.shape[0] > IBD_MAX_PAIRS:
        raise ValueError("%s: the number of pairs must be in [1, 2^27]" % who)
    if not np.array_equal(a.astype(np.int64), a):
        raise ValueError("%s: pairs must be whole numbers" % who)
    a = a.astype(np.int64)
    bad = np.flatnonzero((a[:, 0] < 0) | (a[:, 0] >= a[:, 1]) | (a[:, 1] >= n))
    if bad.size:
        raise ValueError("%s: pair %d is not 0 <= i < j < n" % (who, int(bad[0])))
    return np.ascontiguousarray(a, dtype=np.int32)


def _ibd_args(who, n, nm, pairs, chrom, pos, params):
    ch, ps, _ = _ld_stats_args(who, nm, chrom, pos, 0, None)
    p = ibd_params(who, **params)
    if nm >= 1 << 31:
        raise ValueError("%s: 2^31 markers or more" % who)
    pr = ibd_pairs(who, pairs, n)
    if ps is not None:
        blk = roh_blocks(ch, nm)
        d = np.diff(ps) < 0
        d[blk[1:-1] - 1] = False                         # block edges are not compared across
        if d.any():
            raise ValueError("%s: pos decreases inside a block (panel marker %d)" % (who, int(np.flatnonzero(d)[0]) + 1))
    return pr, ch, ps, _lib.IbdParams(*[p[f] for f in _IBD_FIELDS])


def _ibd_call(fn, device, head, pr, ch, ps, prm, mem, n, seg_cap):
    P = n * (n - 1) // 2 if pr is None else pr.shape[0]
    tab = np.zeros((P, 4), dtype=np.int64)
    while True:
        seg = np.zeros((seg_cap, 6), dtype=np.int32)
        total = C.c_long(0)
        _args_first(fn, device, head + (pr.ctypes.data_as(_c_i32p) if pr is not None else None, P if pr is not None else 0,
                                        ch.ctypes.data_as(_c_i32p) if ch is not None else None,
                                        ps.ctypes.data_as(_c_i64p) if ps is not None else None, C.addressof(prm), float(mem),
                                        tab.ctypes.data_as(_c_i64p), seg.ctypes.data_as(_c_i32p) if seg_cap else None, seg_cap, C.byref(total)))
        if total.value <= seg_cap:
            return tab, seg[:total.value].copy()
        seg_cap = int(total.value)


def ibd(f_name_ascii_M, dims, pairs=None, chrom=None, pos=None, max_memory_in_Gbytes=8.0, device=0, seg_cap=None, **params):
    """eagle_ibd -> (pair int64 (P, 4), seg int32 (S, 6)): the shared-genotype runs of include/eagle_hip.h section 1b'''vii on the
    ingested panel M.ascii (dims = (n, L) of M).  pair = (segments, sum of nsnp, sum of len, longest len) per pair; seg rows = (i, j,
    first marker, last marker, nbreak, block ordinal), sorted by (pair ordinal, first marker).  pairs: int (P, 2) with 0 <= i < j < n,
    duplicates allowed, or None for all pairs in row-major upper-triangle order.  chrom, pos: one whole number per marker or None (one
    block; pos = the marker index).  params: mode (1 / "ibs1", 2 / "ibs2"), min_snp, min_len, max_gap, merge_min (IBD_DEFAULTS).  The
    library is called once with a capacity guess (seg_cap, default 4 P) and once more if that was short.  ValueError for bad arguments
    before the library is called.  r_api.ibd_host is the numpy restatement."""
    L = _lib.load()
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    pr, ch, ps, prm = _ibd_args("ibd", n, nm, pairs, chrom, pos, params)
    P = n * (n - 1) // 2 if pr is None else pr.shape[0]
    cap = 4 * P if seg_cap is None else int(seg_cap)
    if cap < 0:
        raise ValueError("ibd: seg_cap must not be negative")
    return _ibd_call(L.eagle_ibd, device, (os.fsencode(f_name_ascii_M), _dims(dims)), pr, ch, ps, prm, max_memory_in_Gbytes, n, cap)


def bed_ibd(bed_path, dims, include=None, pairs=None, chrom=None, pos=None, availmemGb=8.0, device=0, seg_cap=None, **params):
    """eagle_bed_ibd -> ibd's pair of tables by PANEL marker from a SNP-major PLINK .bed file of dims = (n individuals, L markers), which
    still knows its missing calls: a marker where either individual is not called (code 01) is never a break.  include as in
    bed_ld_window; chrom and pos: one whole number per panel marker."""
    L = _lib.load()
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    inc = _bed_ld_include(include, nm, "bed_ibd")
    linc = nm if inc is None else int(inc.sum())
    pr, ch, ps, prm = _ibd_args("bed_ibd", n, linc, pairs, chrom, pos, params)
    P = n * (n - 1) // 2 if pr is None else pr.shape[0]
    cap = 4 * P if seg_cap is None else int(seg_cap)
    if cap < 0:
        raise ValueError("bed_ibd: seg_cap must not be negative")
    head = (os.fsencode(bed_path), _dims(dims), inc.ctypes.data_as(C.c_void_p) if inc is not None else None)
    return _ibd_call(L.eagle_bed_ibd, device, head, pr, ch, ps, prm, availmemGb, n, cap)


# ---- Mendel errors and parentage assignment (include/eagle_hip.h section 1b'''viii): exact integers on the IBD bit planes ----
MENDEL_MAX_TRIOS = 1 << 27


def _whole_int32(who, what, x, ndim):
    a = np.asarray(x)
    if a.ndim != ndim:
        raise ValueError("%s: %s must be a %d-dimensional list of whole numbers" % (who, what, ndim))
    if a.size == 0:
        return np.zeros(a.shape, dtype=np.int32)
    if a.dtype == bool or a.dtype.kind not in "iuf":
        raise ValueError("%s: %s must be whole numbers" % (who, what))
    if not np.all(np.isfinite(a)) or not np.array_equal(np.floor(a), a) or a.min() < -(1 << 31) or a.max() >= 1 << 31:
        raise ValueError("%s: %s must be whole numbers that fit int32" % (who, what))
    return np.ascontiguousarray(a, dtype=np.int32)


def mendel_trios(who, trios, n):
    """A trio list as contiguous int32 (T, 3) of (child, father, mother); ValueError for a count outside [1, 2^27] or a trio that is not
    0 <= c < n, -1 <= f, m < n (-1: unknown), c != f, c != m, f != m unless both are -1."""
    a = np.asarray(trios)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1 or a.shape[0] > MENDEL_MAX_TRIOS:
        raise ValueError("%s: the number of trios must be in [1, 2^27] (rows of child, father, mother)" % who)
    t = _whole_int32(who, "trios", a, 2).astype(np.int64)
    c, f, m = t[:, 0], t[:, 1], t[:, 2]
    bad = np.flatnonzero((c < 0) | (c >= n) | (f < -1) | (f >= n) | (m < -1) | (m >= n) | (c == f) | (c == m) | ((f == m) & (f >= 0)))
    if bad.size:
        raise ValueError("%s: trio %d is not (c, f, m) with 0 <= c < n, -1 <= f, m < n, c != f, c != m, f != m" % (who, int(bad[0])))
    return np.ascontiguousarray(t, dtype=np.int32)


def parentage_lists(who, offspring, sires, dams, n, min_overlap=1, allow_self=False):
    """The three index lists of a parentage call as contiguous int32 (None or empty: no list), min_overlap and allow_self as ints;
    ValueError for an index outside [0, n), a duplicate inside a list, no offspring, both candidate lists empty, sires x dams >= 2^31,
    a min_overlap outside [0, 2^31) or an allow_self that is not a truth value."""
    out = []
    for what, x in (("offspring", offspring), ("sires", sires), ("dams", dams)):
        a = _whole_int32(who, what, [] if x is None else x, 1)
        if a.size and (a.min() < 0 or a.max() >= n):
            raise ValueError("%s: %s entry %d is outside [0, n)" % (who, what, int(np.flatnonzero((a < 0) | (a >= n))[0])))
        if np.unique(a).size != a.size:
            raise ValueError("%s: %s holds a duplicate" % (who, what))
        out.append(a)
    o, s, d = out
    if o.size < 1 or o.size > MENDEL_MAX_TRIOS:
        raise ValueError("%s: the number of offspring must be in [1, 2^27]" % who)
    if s.size == 0 and d.size == 0:
        raise ValueError("%s: both candidate lists are empty" % who)
    if max(s.size, 1) * max(d.size, 1) >= 1 << 31:
        raise ValueError("%s: sires x dams must be below 2^31" % who)
    try:
        mo = int(min_overlap)
    except (TypeError, ValueError):
        raise ValueError("%s: min_overlap must be a whole number" % who)
    if mo != min_overlap or not 0 <= mo < 1 << 31:
        raise ValueError("%s: min_overlap must be a whole number in [0, 2^31)" % who)
    if allow_self not in (0, 1, False, True):
        raise ValueError("%s: allow_self must be 0 or 1" % who)
    return o, s, d, mo, int(bool(allow_self))


def _mendel_call(fn, device, head, tr, nm, mem, markers):
    out = np.zeros((tr.shape[0], 6), dtype=np.int32)
    mk = np.zeros(nm, dtype=np.int32) if markers else None
    _args_first(fn, device, head + (tr.ctypes.data_as(_c_i32p), tr.shape[0], float(mem), out.ctypes.data_as(_c_i32p),
                                    mk.ctypes.data_as(_c_i32p) if markers else None))
    return out, mk


def mendel(f_name_ascii_M, dims, trios, max_memory_in_Gbytes=8.0, device=0, markers=True):
    """eagle_mendel -> (trio int32 (T, 6), marker int32 (L) or None): the Mendel errors of include/eagle_hip.h section 1b'''viii on the
    ingested panel M.ascii (dims = (n, L) of M).  trios: int (T, 3) of (child, father, mother) individual indices, -1 = unknown parent.
    trio rows = (n_cf, e_cf, n_cm, e_cm, n_trio, e): markers called in child and father, their opposite homozygotes, the same for the
    mother, markers called in all three, Mendel errors.  marker = the trios of the list with an error at each marker (markers=False:
    not computed).  ValueError for bad arguments before the library is called.  r_api.mendel_host is the numpy restatement."""
    L = _lib.load()
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    tr = mendel_trios("mendel", trios, n)
    if nm >= 1 << 31:
        raise ValueError("mendel: 2^31 markers or more")
    return _mendel_call(L.eagle_mendel, device, (os.fsencode(f_name_ascii_M), _dims(dims)), tr, nm, max_memory_in_Gbytes, markers)


def bed_mendel(bed_path, dims, trios, include=None, availmemGb=8.0, device=0, markers=True):
    """eagle_bed_mendel -> mendel's pair by PANEL marker from a SNP-major PLINK .bed file of dims = (n individuals, L markers), which
    still knows its missing calls: a child that is not called has no error, a parent that is not called can pass either allele.
    include as in bed_ld_window."""
    L = _lib.load()
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    inc = _bed_ld_include(include, nm, "bed_mendel")
    linc = nm if inc is None else int(inc.sum())
    tr = mendel_trios("bed_mendel", trios, n)
    head = (os.fsencode(bed_path), _dims(dims), inc.ctypes.data_as(C.c_void_p) if inc is not None else None)
    return _mendel_call(L.eagle_bed_mendel, device, head, tr, linc, availmemGb, markers)


def _parentage_call(fn, device, head, lists, mem):
    o, s, d, mo, selfing = lists
    best = np.zeros((o.size, 2, 4), dtype=np.int32)
    _args_first(fn, device, head + (o.ctypes.data_as(_c_i32p), o.size, s.ctypes.data_as(_c_i32p) if s.size else None, s.size,
                                    d.ctypes.data_as(_c_i32p) if d.size else None, d.size, mo, selfing, float(mem), best.ctypes.data_as(_c_i32p)))
    return best


def parentage(f_name_ascii_M, dims, offspring, sires=None, dams=None, min_overlap=1, allow_self=False, max_memory_in_Gbytes=8.0, device=0):
    """eagle_parentage -> int32 (n_o, 2, 4): per offspring the best and the runner-up candidate (sire, dam, Mendel errors, overlap) of the
    exhaustive search over sires x dams (include/eagle_hip.h section 1b'''viii rule 6) on the ingested panel M.ascii (dims = (n, L) of
    M), as individual indices; -1 rows where there is no such candidate.  An empty (or None) list is one unknown parent.  The rank is
    by error count, ties to the earlier candidate.  ValueError for bad arguments before the library is called.  r_api.parentage_host is
    the numpy restatement."""
    L = _lib.load()
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    lists = parentage_lists("parentage", offspring, sires, dams, n, min_overlap, allow_self)
    if nm >= 1 << 31:
        raise ValueError("parentage: 2^31 markers or more")
    return _parentage_call(L.eagle_parentage, device, (os.fsencode(f_name_ascii_M), _dims(dims)), lists, max_memory_in_Gbytes)


def bed_parentage(bed_path, dims, offspring, sires=None, dams=None, include=None, min_overlap=1, allow_self=False, availmemGb=8.0, device=0):
    """eagle_bed_parentage -> parentage's rows by PANEL marker from a SNP-major PLINK .bed file, where the overlap of a candidate is the
    number of markers called in the child and both parents (the known one, in single-parent assignment) and must reach min_overlap."""
    L = _lib.load()
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    inc = _bed_ld_include(include, nm, "bed_parentage")
    lists = parentage_lists("bed_parentage", offspring, sires, dams, n, min_overlap, allow_self)
    head = (os.fsencode(bed_path), _dims(dims), inc.ctypes.data_as(C.c_void_p) if inc is not None else None)
    return _parentage_call(L.eagle_bed_parentage, device, head, lists, availmemGb)


# ---- GRM (include/eagle_hip.h section 1b''''): the exact weighted Gram product; weights, centring and PCA are r_api's ----
WGRAM_MAX_WEIGHT = (1 << 21) - 1


def weighted_gram(f_name_ascii_M, dims, q, max_memory_in_Gbytes=8.0, device=0):
    """eagle_weighted_gram -> int64 (n, n): Q_ij = sum over the markers m of q_m g_im g_jm with g in {-1, 0, +1}, exact, for integer
    weights 0 <= q_m <= WGRAM_MAX_WEIGHT = 2^21 - 1, one per marker of M.ascii (dims = (n, L) of M).  ValueError for a q of another
    length, a negative, fractional or too large weight, before the library is called.  A view alias gives the matrix of its kept
    individuals."""
    L = _lib.load()
    n, nm = int(dims[0]), int(dims[1])
    qa = np.atleast_1d(np.asarray(q)).ravel()
    if qa.size != nm:
        raise ValueError("weighted_gram: q holds %d weights, the panel %d markers" % (qa.size, nm))
    if qa.dtype == bool:
        qa = qa.astype(np.int64)
    if qa.dtype.kind not in "iu":
        if qa.dtype.kind != "f" or not np.all(qa == np.floor(qa)):   # (a NaN fails the comparison)
            raise ValueError("weighted_gram: q must hold whole numbers")
    if qa.size and qa.min() < 0:
        raise ValueError("weighted_gram: a weight is negative")
    if qa.size and qa.max() > WGRAM_MAX_WEIGHT:
        raise ValueError("weighted_gram: a weight is 2^21 or more")
    q32 = np.ascontiguousarray(qa, dtype=np.uint32)
    out = np.zeros((n, n), dtype=np.int64)
    _args_first(L.eagle_weighted_gram, device, (os.fsencode(f_name_ascii_M), _dims(dims), q32.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                float(max_memory_in_Gbytes), out.ctypes.data_as(C.POINTER(C.c_int64))))
    return out


# ---- line scores (include/eagle_hip.h section 1b''''i): M w and M^T V as exact integers; quantising and scaling are r_api's ----
SCORES_MAX_COLUMNS = 64
SCORES_MAX_WEIGHT = 1 << 30
SCORES_MAX_LINE = 8388480


def _score_weights(who, w, length):
    """The weights of a scores call as int64 (T, length); ValueError before the library is called."""
    wa = np.asarray(w)
    if wa.ndim == 1:
        wa = wa[None, :]
    if wa.ndim != 2 or wa.shape[0] < 1 or wa.shape[1] != length:
        raise ValueError("%s: the weights must be (%d,) or (T, %d), got %s" % (who, length, length, np.shape(w)))
    if wa.dtype == bool:
        wa = wa.astype(np.int64)
    if wa.dtype.kind not in "iu":
        if wa.dtype.kind != "f" or not np.all(wa == np.floor(wa)):   # (a NaN fails the comparison)
            raise ValueError("%s: the weights must hold whole numbers" % who)
    if wa.size and (wa.max() > SCORES_MAX_WEIGHT or wa.min() < -SCORES_MAX_WEIGHT):
        raise ValueError("%s: a weight is beyond +-2^30" % who)
    return wa.astype(np.int64)


def _line_scores(fn, who, path, dims, rows, length, w, max_memory_in_Gbytes, device):
    wa = _score_weights(who, w, length)
    out = np.zeros((rows, wa.shape[0]), dtype=np.int64)
    for t0 in range(0, wa.shape[0], SCORES_MAX_COLUMNS):   # more than 64 columns: calls of 64
        w32 = np.ascontiguousarray(wa[t0:t0 + SCORES_MAX_COLUMNS], dtype=np.int32)
        part = np.zeros((rows, w32.shape[0]), dtype=np.int64)
        _args_first(fn, device, (os.fsencode(path), _dims(dims), w32.ctypes.data_as(_c_i32p), w32.shape[0], float(max_memory_in_Gbytes),
                                 part.ctypes.data_as(_c_i64p)))
        out[:, t0:t0 + w32.shape[0]] = part
    return out


def sample_scores(f_name_ascii_M, dims, w, max_memory_in_Gbytes=8.0, device=0):
    """eagle_sample_scores -> int64 (n, T): S[i, t] = sum over the markers m of w[t, m] g_im with g in {-1, 0, +1}, exact, for integer
    weights |w| <= SCORES_MAX_WEIGHT = 2^30; w is (L,) (T = 1) or (T, L) of any integer dtype (dims = (n, L) of M).  ValueError for a
    wrong length, a fractional value or a weight beyond 2^30, before the library is called.  More than SCORES_MAX_COLUMNS columns run
    as calls of 64.  A view alias gives the scores of its kept individuals.  r_api.line_scores_host is the numpy restatement."""
    L = _lib.load()
    return _line_scores(L.eagle_sample_scores, "sample_scores", f_name_ascii_M, dims, max(int(dims[0]), 0), max(int(dims[1]), 0), w,
                        max_memory_in_Gbytes, device)


def marker_scores(f_name_ascii_Mt, dims, v, max_memory_in_Gbytes=8.0, device=0):
    """eagle_marker_scores -> int64 (L, T): the exact M^T V, out[m, t] = sum over the individuals i of v[t, i] g_im, for integer weights
    |v| <= 2^30; v is (n,) or (T, n) (dims = (n, L) of M).  For a view alias n = dims[0] is the number of kept individuals."""
    L = _lib.load()
    return _line_scores(L.eagle_marker_scores, "marker_scores", f_name_ascii_Mt, dims, max(int(dims[1]), 0), max(int(dims[0]), 0), v,
                        max_memory_in_Gbytes, device)


# ---- epistasis (include/eagle_hip.h section 1b''''ii): exact sums and the F statistic; p-values and effects are r_api's ----
EPI_MAX_N = 65535
EPI_YMAX = 1000000


class EpiMax(C.Structure):
    """eagle_epi_max of include/eagle_hip.h section 1b''''ii."""
    _fields_ = [("i", C.c_int64), ("j", C.c_int64), ("stat", C.c_double)]


def _epi_trait(who, y, n):
    ya = np.asarray(y)
    if ya.ndim != 1 or ya.size != n or not np.issubdtype(ya.dtype, np.integer):
        raise ValueError("%s: y must hold one integer per individual (%d); r_api.quantise_trait makes one from a real trait" % (who, n))
    if ya.size and int(np.abs(ya.astype(np.int64)).max()) > EPI_YMAX:
        raise ValueError("%s: a trait value beyond EPI_YMAX = %d in absolute value" % (who, EPI_YMAX))
    return np.ascontiguousarray(ya, dtype=np.int32)


def epistasis_loci(f_name_ascii_Mt, dims, y, loci, max_memory_in_Gbytes=8.0, device=0, moments=True):
    """eagle_epistasis_loci -> (stat fp64 (L, k), mom int64 (L, k, 5) or None): the F(1, n - 4) of the interaction of every marker i with
    the k <= 64 markers loci (0-based, repeats allowed) for the integer trait y (|y| <= EPI_YMAX; dims = (n, L) of M, n <= EPI_MAX_N), NaN
    where the pair is undefined, and the five pair sums (d, e, f, h, z).  r_api.epistasis_host is the numpy restatement."""
    L = _lib.load()
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    yv = _epi_trait("epistasis_loci", y, n)
    lv = np.ascontiguousarray(np.atleast_1d(np.asarray(loci, dtype=np.int64)).ravel(), dtype=np.int64)
    if lv.size and not np.all(np.asarray(loci).ravel() == lv):
        raise ValueError("epistasis_loci: loci must hold whole numbers")
    k = max(int(lv.size), 1)
    stat = np.zeros((nm, k), dtype=np.float64)
    mom = np.zeros((nm, k, 5), dtype=np.int64) if moments else None
    _args_first(L.eagle_epistasis_loci, device, (os.fsencode(f_name_ascii_Mt), _dims(dims), yv.ctypes.data_as(_c_i32p), lv.ctypes.data_as(c_lp),
                                                 lv.size, float(max_memory_in_Gbytes), stat.ctypes.data_as(c_dp),
                                                 mom.ctypes.data_as(_c_i64p) if moments else None))
    return stat, mom


def epistasis_pairs(f_name_ascii_Mt, dims, y, chrom=None, gap=0, min_stat=0.0, hit_cap=1 << 20, max_memory_in_Gbytes=8.0, device=0):
    """eagle_epistasis_pairs -> {"nhits", "ntested", "max": (i, j, stat), "hit_ij" int32 (nhits, 2), "hit_stat" fp64 (nhits), "hit_mom"
    int64 (nhits, 5)}: all pairs i < j of the resident panel except those at most `gap` markers apart on one chromosome (chrom: one whole
    number per marker, or None = one chromosome), a hit where stat >= min_stat, the tables sorted by (i, j).  With more than hit_cap hits the
    three tables are None and nhits still holds the total (one call, eagle_roh's capacity rule)."""
    L = _lib.load()
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    yv = _epi_trait("epistasis_pairs", y, n)
    ch = None
    if chrom is not None:
        ca = np.asarray(chrom).ravel()
        if ca.size != nm or not np.all(ca == np.rint(ca.astype(np.float64))):
            raise ValueError("epistasis_pairs: chrom must hold one whole number per marker")
        ch = np.ascontiguousarray(ca, dtype=np.int32)
    cap = int(hit_cap)
    if cap < 0 or int(gap) != gap or gap < 0 or min_stat != min_stat:
        raise ValueError("epistasis_pairs: hit_cap and gap must not be negative, min_stat not NaN")
    ij, st, mom = np.zeros((cap, 2), dtype=np.int32), np.zeros(cap, dtype=np.float64), np.zeros((cap, 5), dtype=np.int64)
    nh, nt, mx = C.c_long(0), C.c_long(0), EpiMax(-1, -1, float("nan"))
    _args_first(L.eagle_epistasis_pairs, device, (os.fsencode(f_name_ascii_Mt), _dims(dims), yv.ctypes.data_as(_c_i32p),
                                                  ch.ctypes.data_as(_c_i32p) if ch is not None else None, int(gap), float(min_stat),
                                                  float(max_memory_in_Gbytes), ij.ctypes.data_as(_c_i32p) if cap else None,
                                                  st.ctypes.data_as(c_dp) if cap else None, mom.ctypes.data_as(_c_i64p) if cap else None, cap,
                                                  C.byref(nh), C.byref(nt), C.addressof(mx)))
    out = {"nhits": int(nh.value), "ntested": int(nt.value), "max": (int(mx.i), int(mx.j), float(mx.stat)), "hit_ij": None, "hit_stat": None,
           "hit_mom": None}
    if out["nhits"] <= cap:
        out.update(hit_ij=ij[:out["nhits"]].copy(), hit_stat=st[:out["nhits"]].copy(), hit_mom=mom[:out["nhits"]].copy())
    return out


# ---- per-group genotype counts and Fisher's exact test (include/eagle_hip.h section 1b''''iii); the statistics are r_api's ----
GROUPS_MAX = 64


def _group_labels(who, labels, n, K):
    """labels as int64 (n) and the number of groups: whole numbers in [-1, K), K = max + 1 (at least 1) when not given."""
    la = np.asarray(labels)
    if la.ndim != 1 or la.size != n:
        raise ValueError("%s: labels must hold one entry per individual (%d)" % (who, n))
    if la.dtype.kind not in "iuf" or not np.all(np.isfinite(la.astype(np.float64))) or not np.all(la == np.rint(la.astype(np.float64))):
        raise ValueError("%s: labels must hold whole numbers (-1 = in no group)" % who)
    lv = la.astype(np.int64)
    if K is None:
        K = max(int(lv.max()) + 1, 1) if lv.size else 1
    if int(K) != K or K < 1:
        raise ValueError("%s: K must be a whole number of at least 1" % who)
    if lv.size and (int(lv.min()) < -1 or int(lv.max()) >= K):
        raise ValueError("%s: a label outside [-1, K = %d)" % (who, K))
    return lv, int(K)


def _group_rounds(fn, who, path, dims, labels, K, width, max_memory_in_Gbytes, device):
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    lv, K = _group_labels(who, labels, n, K)
    L = _lib.load()
    out = np.zeros((nm, K, width), dtype=np.int32)
    for k0 in range(0, K, GROUPS_MAX):                  # rounds of 64 groups, the others in no group: a partition makes this exact
        kr = min(GROUPS_MAX, K - k0)
        lr = np.ascontiguousarray(np.where((lv >= k0) & (lv < k0 + kr), lv - k0, -1), dtype=np.int32)
        part = out if K <= GROUPS_MAX else np.zeros((nm, kr, width), dtype=np.int32)
        _args_first(getattr(L, fn), device, (os.fsencode(path), _dims(dims), lr.ctypes.data_as(_c_i32p), kr, float(max_memory_in_Gbytes),
                                             part.ctypes.data_as(_c_i32p)))
        if part is not out:
            out[:, k0:k0 + kr] = part
    return out


def group_counts(f_name_ascii_Mt, dims, labels, K=None, max_memory_in_Gbytes=8.0, device=0):
    """eagle_group_counts -> int32 (L, K, 3): the numbers of '0', '1', '2' characters of every line of Mt.ascii (dims = (n, L) of M) among
    the individuals of every group; labels = one whole number in [-1, K) per individual (-1 = in no group; with a view alias one per kept
    individual), K = max(labels) + 1 when not given.  More than 64 groups run as rounds of 64.  r_api.group_counts_host restates it."""
    return _group_rounds("eagle_group_counts", "group_counts", f_name_ascii_Mt, dims, labels, K, 3, max_memory_in_Gbytes, device)


def bed_group_counts(bed_path, dims, labels, K=None, max_memory_in_Gbytes=8.0, device=0):
    """eagle_bed_group_counts -> int32 (L, K, 4): homozygous A1, heterozygous, homozygous A2, missing of every marker of a SNP-major PLINK
    .bed file of dims = (n individuals, L markers) among the individuals of every group (labels and K as in group_counts)."""
    return _group_rounds("eagle_bed_group_counts", "bed_group_counts", bed_path, dims, labels, K, 4, max_memory_in_Gbytes, device)


def fisher_2x2(tables, device=0):
    """eagle_fisher_2x2 -> fp64 (L): the two-sided Fisher exact test of tables = int (L, 4) rows (a, b, c, d) of the 2 x 2 tables
    (a, b; c, d), entries >= 0 and sums <= 2^30, in the fixed order of the header (r_api.fisher_2x2_host gives the same bits)."""
    t = np.asarray(tables)
    if t.ndim != 2 or t.shape[1] != 4 or t.shape[0] < 1:
        raise ValueError("fisher_2x2: tables must be (L, 4) with L >= 1")
    t32 = np.ascontiguousarray(t, dtype=np.int32)
    if not np.array_equal(t32, t):
        raise ValueError("fisher_2x2: tables must hold whole numbers that fit int32")
    if int(t32.min()) < 0 or int(t32.astype(np.int64).sum(axis=1).max()) > 1 << 30:
        raise ValueError("fisher_2x2: entries must not be negative and a table must not sum to more than 2^30")
    out = np.zeros(t32.shape[0], dtype=np.float64)
    _args_first(_lib.load().eagle_fisher_2x2, device, (t32.ctypes.data_as(_c_i32p), t32.shape[0], _dp(out)))
    return out


# ---- max(T) permutation testing (include/eagle_hip.h section 1b''''vi); the statistics and p-values are r_api's ----
MAXT_MAX_N = 65535
MAXT_TMAX = 1000000
MAXT_RMAX = 1024


def maxt(fMt, dims, t, used=None, strata=None, seed=0, first=1, R=1000, perm=None, availmemGb=8, device=0):
    """eagle_maxt -> {"d_obs" int64 (L), "V" int64 (L), "key_obs" fp64 (L), "count1" int32 (L), "maxkey" fp64 (R), "argmax" int32 (R)}: the
    raw outputs of section 1b''''vi for the permutations first .. first + R - 1 of an integer trait t (|t| <= 10^6, one entry per
    individual of Mt.ascii, dims = (n, L) of M).  used: a mask of the individuals that take part (None: all); strata: whole numbers in
    [0, 2^16) within which the seeded permutations stay; perm: int (R, N) explicit permutations of the used individuals instead of the
    seeded ones.  More than MAXT_RMAX = 1024 permutations run as several calls of the library, whose count1 add and whose maxkey and
    argmax concatenate.  r_api.maxt_host restates it: the same words."""
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    first, R = int(first), int(R)

    def whole(name, a, size, lo, hi):
        v = np.asarray(a)
        if v.ndim != 1 or v.size != size:
            raise ValueError("maxt: %s must hold one entry per individual (%d)" % (name, size))
        if v.dtype.kind not in "iufb" or not np.all(np.isfinite(v.astype(np.float64))) or not np.all(v == np.rint(v.astype(np.float64))):
            raise ValueError("maxt: %s must hold whole numbers" % name)
        return np.ascontiguousarray(np.clip(v.astype(np.int64), lo, hi), dtype=np.int32)

    tv = whole("t", t, n, -MAXT_TMAX - 1, MAXT_TMAX + 1)                  # beyond the limit stays beyond it: the library's error
    uv = None
    if used is not None:
        uv = np.asarray(used)
        if uv.ndim != 1 or uv.size != n:
            raise ValueError("maxt: used must hold one entry per individual (%d)" % n)
        uv = np.ascontiguousarray(uv.astype(bool), dtype=np.uint8)
    sv = None if strata is None else whole("strata", strata, n, -1, 65536)
    N = n if uv is None else int(uv.sum())
    pv = None
    if perm is not None:
        pa = np.asarray(perm)
        if pa.ndim != 2 or pa.shape != (R, N) or pa.dtype.kind not in "iu":
            raise ValueError("maxt: perm must be whole numbers of shape (R, N) = (%d, %d)" % (R, N))
        pv = np.ascontiguousarray(np.clip(pa.astype(np.int64), -1, N), dtype=np.int32)
    L = _lib.load()
    u8p = C.POINTER(C.c_uint8)
    out = {"d_obs": np.zeros(nm, dtype=np.int64), "V": np.zeros(nm, dtype=np.int64), "key_obs": np.zeros(nm, dtype=np.float64),
           "count1": np.zeros(nm, dtype=np.int32), "maxkey": np.zeros(max(R, 0), dtype=np.float64), "argmax": np.zeros(max(R, 0), dtype=np.int32)}
    r0 = 0
    while True:
        nr = R - r0 if R <= 0 else min(MAXT_RMAX, R - r0)                # R <= 0 goes through once: the library's error
        c1 = np.zeros(nm, dtype=np.int32)
        mk, am = np.zeros(max(nr, 1), dtype=np.float64), np.zeros(max(nr, 1), dtype=np.int32)
        pc = None if pv is None else np.ascontiguousarray(pv[r0:r0 + nr])
        _args_first(L.eagle_maxt, device, (os.fsencode(fMt), _dims(dims), tv.ctypes.data_as(_c_i32p), None if uv is None else uv.ctypes.data_as(u8p),
                                           None if sv is None else sv.ctypes.data_as(_c_i32p), C.c_uint64(int(seed) & (2 ** 64 - 1)), first + r0, nr,
                                           None if pc is None else pc.ctypes.data_as(_c_i32p), float(availmemGb),
                                           out["d_obs"].ctypes.data_as(_c_i64p), out["V"].ctypes.data_as(_c_i64p), _dp(out["key_obs"]),
                                           c1.ctypes.data_as(_c_i32p), _dp(mk), am.ctypes.data_as(_c_i32p)))
        out["count1"] += c1
        out["maxkey"][r0:r0 + nr], out["argmax"][r0:r0 + nr] = mk[:nr], am[:nr]
        r0 += nr
        if r0 >= R:
            return out


# ---- transmission disequilibrium test of trios (include/eagle_hip.h section 1b''''viii); the statistics and p-values are r_api's ----
TDT_MAX_FLIP_TRIOS = 65535


def tdt_args(who, trios, n, nm, family, seed, first, R):
    """The arguments of a TDT call checked without the library -> (trios int32 (T, 3), family int32 (T) or None, seed, first, R) as the
    library takes them; ValueError for what section 1b''''viii calls an argument error: mendel_trios' rule, 2^31 markers or more, a
    negative R, first < 1, first + R > 2^31, more than 65,535 trios with R >= 1, a family list that is not one whole number in
    [0, 65535] per trio."""
    tr = mendel_trios(who, trios, n)
    if nm >= 1 << 31:
        raise ValueError("%s: 2^31 markers or more" % who)
    try:
        Ri, fi, sd = int(R), int(first), int(seed)
    except (TypeError, ValueError):
        raise ValueError("%s: R, first and seed must be whole numbers" % who)
    if Ri != R or fi != first or sd != seed or Ri < 0:
        raise ValueError("%s: R, first and seed must be whole numbers, R not negative" % who)
    fam = None
    if Ri >= 1:
        if fi < 1 or fi + Ri > 1 << 31:
            raise ValueError("%s: first must be at least 1 and first + R at most 2^31" % who)
        if tr.shape[0] > TDT_MAX_FLIP_TRIOS:
            raise ValueError("%s: more than 65535 trios with flips (R >= 1)" % who)
        if family is not None:
            fam = _whole_int32(who, "family", family, 1)
            if fam.size != tr.shape[0] or (fam.size and (fam.min() < 0 or fam.max() > 65535)):
                raise ValueError("%s: family must hold one whole number in [0, 65535] per trio" % who)
    return tr, fam, sd & (2 ** 64 - 1), fi, Ri


def _tdt_call(fn, device, head, tr, fam, seed, first, R, nm, mem):
    T = tr.shape[0]
    out = {"trio": np.zeros((T, 6), dtype=np.int32), "marker": np.zeros((nm, 5), dtype=np.int32), "key_obs": np.zeros(nm, dtype=np.float64),
           "count1": np.zeros(nm, dtype=np.int32), "maxkey": np.zeros(R, dtype=np.float64), "argmax": np.zeros(R, dtype=np.int32)}
    r0 = 0
    while True:
        nr = min(MAXT_RMAX, R - r0)
        c1 = np.zeros(nm, dtype=np.int32)
        mk, am = np.zeros(max(nr, 1), dtype=np.float64), np.zeros(max(nr, 1), dtype=np.int32)
        _args_first(fn, device, head + (tr.ctypes.data_as(_c_i32p), T, None if fam is None else fam.ctypes.data_as(_c_i32p), C.c_uint64(seed),
                                        first + r0, nr, float(mem), out["trio"].ctypes.data_as(_c_i32p), out["marker"].ctypes.data_as(_c_i32p),
                                        _dp(out["key_obs"]), c1.ctypes.data_as(_c_i32p), _dp(mk), am.ctypes.data_as(_c_i32p)))
        out["count1"] += c1
        out["maxkey"][r0:r0 + nr], out["argmax"][r0:r0 + nr] = mk[:nr], am[:nr]
        r0 += nr
        if r0 >= R:
            return out


def tdt(f_name_ascii_M, dims, trios, family=None, seed=0, first=1, R=0, max_memory_in_Gbytes=8.0, device=0):
    """eagle_tdt -> {"trio" int32 (T, 6), "marker" int32 (L, 5), "key_obs" fp64 (L), "count1" int32 (L), "maxkey" fp64 (R), "argmax" int32
    (R)}: the raw outputs of include/eagle_hip.h section 1b''''viii on the ingested panel M.ascii (dims = (n, L) of M).  trios: int (T, 3)
    of (child, father, mother), -1 = unknown parent.  trio rows = (complete markers, informative het fathers, informative het mothers,
    T_t, U_t, W_t); marker rows = (PT, PU, MT, MU, W) summed over the list; key_obs = the TDT chi-square (T - U)^2 / (T + U).  R = 0:
    counts only.  R >= 1: the flips first .. first + R - 1 of the families (family: one whole number in [0, 65535] per trio; None: trios
    with the same parents are one family); more than MAXT_RMAX = 1024 flips run as several calls of the library, whose count1 add and
    whose maxkey and argmax concatenate.  ValueError for bad arguments before the library is loaded.  r_api.tdt_host restates it."""
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    tr, fam, sd, fi, Ri = tdt_args("tdt", trios, n, nm, family, seed, first, R)
    L = _lib.load()
    return _tdt_call(L.eagle_tdt, device, (os.fsencode(f_name_ascii_M), _dims(dims)), tr, fam, sd, fi, Ri, nm, max_memory_in_Gbytes)


def bed_tdt(bed_path, dims, trios, include=None, family=None, seed=0, first=1, R=0, availmemGb=8.0, device=0):
    """eagle_bed_tdt -> tdt's dict by PANEL marker from a SNP-major PLINK .bed file of dims = (n individuals, L markers), which still knows
    its missing calls: a trio with a missing call at a marker is not complete there.  include as in bed_ld_window."""
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    inc = _bed_ld_include(include, nm, "bed_tdt")
    linc = nm if inc is None else int(inc.sum())
    tr, fam, sd, fi, Ri = tdt_args("bed_tdt", trios, n, linc, family, seed, first, R)
    L = _lib.load()
    head = (os.fsencode(bed_path), _dims(dims), inc.ctypes.data_as(C.c_void_p) if inc is not None else None)
    return _tdt_call(L.eagle_bed_tdt, device, head, tr, fam, sd, fi, Ri, linc, availmemGb)


# ---- pairwise haplotype EM and D' (include/eagle_hip.h section 1b''''vii); the blocks are r_api's ----
def hap_ld(fMt, dims, window=50, tol=1e-10, max_iter=1000, fg_cut=0.01, dprime_cut=0.8, bands=False, masks=True, availmemGb=8, device=0):
    """eagle_hap_ld -> {"recomb", "strong": uint64 (L, ceil(window / 64)), bit (o - 1) % 64 of word (o - 1) // 64 of row i = the verdict
    on the pair of markers (i, i + o), 1 <= o <= window; with bands=True also "dprime" and "r2": fp64 (L, window), entry (i, o - 1), -2.0 /
    -1.0 for an undefined pair; "counts": int64 (4) = the defined pairs, the pairs whose EM stopped at max_iter, the recombinant bits,
    the strong bits}: the haplotype frequencies of every pair by EM from the unphased genotypes of Mt.ascii (dims = (n, L) of M), the
    rule of section 1b''''vii.  masks=False leaves the two masks out.  r_api.hap_ld_host restates it: the same words."""
    L = _lib.load()
    nm, w = max(int(dims[1]), 0), int(window)
    out = {"counts": np.zeros(4, dtype=np.int64)}
    if masks:
        out["recomb"] = np.zeros((nm, (w + 63) // 64 if w > 0 else 1), dtype=np.uint64)
        out["strong"] = np.zeros_like(out["recomb"])
    if bands:
        out["dprime"] = np.zeros((nm, max(w, 1)), dtype=np.float64)
        out["r2"] = np.zeros_like(out["dprime"])
    _args_first(L.eagle_hap_ld, device, (os.fsencode(fMt), _dims(dims), w, float(tol), int(max_iter), float(fg_cut), float(dprime_cut),
                                         float(availmemGb), out["recomb"].ctypes.data_as(_c_u64p) if masks else None,
                                         out["strong"].ctypes.data_as(_c_u64p) if masks else None, _dp(out["dprime"]) if bands else None,
                                         _dp(out["r2"]) if bands else None, out["counts"].ctypes.data_as(_c_i64p)))
    return out


# ---- logistic regression per marker with covariates (include/eagle_hip.h section 1b''''iv); the p-values are r_api's ----
LOGISTIC_MAX_COVARIATES = 15


def _logistic_inputs(who, n, status, X, beta0, firth, tol, max_iter):
    """(status int32 (n), X fp64 (n, c) column-major, beta0 fp64 (c) or None) after the checks eagle_logistic makes, as ValueError."""
    sa = np.asarray(status)
    if sa.ndim != 1 or sa.size != n:
        raise ValueError("%s: status must hold one entry per individual (%d)" % (who, n))
    if sa.dtype.kind not in "iuf" or not np.all(np.isin(sa, (-1, 0, 1))):
        raise ValueError("%s: status must be 1 (case), 0 (control) or -1 (not used)" % who)
    sv = np.ascontiguousarray(sa, dtype=np.int32)
    Xa = np.asarray(X)
    if Xa.dtype.kind not in "iuf" or Xa.ndim != 2 or Xa.shape[0] != n or not 1 <= Xa.shape[1] <= LOGISTIC_MAX_COVARIATES:
        raise ValueError("%s: X must be numeric (%d, c) with 1 <= c <= %d, the intercept column included" % (who, n, LOGISTIC_MAX_COVARIATES))
    Xf = _f64F(Xa)
    used = sv >= 0
    if not np.all(np.isfinite(Xf[used])):
        raise ValueError("%s: X must be finite on the used individuals" % who)
    if not (sv == 1).any() or not (sv == 0).any():
        raise ValueError("%s: no case or no control among the used individuals" % who)
    if firth not in (0, 1, 2) or isinstance(firth, bool):
        raise ValueError("%s: firth must be 0 (ML), 1 (Firth) or 2 (fallback)" % who)
    if not 0.0 < float(tol) < 1.0:
        raise ValueError("%s: tol must lie in (0, 1)" % who)
    if int(max_iter) != max_iter or not 1 <= max_iter <= 1000:
        raise ValueError("%s: max_iter must be a whole number in [1, 1000]" % who)
    b0 = None
    if beta0 is not None:
        b0 = np.ascontiguousarray(np.asarray(beta0, dtype=np.float64).ravel())
        if b0.size != Xf.shape[1] or not np.all(np.isfinite(b0)):
            raise ValueError("%s: beta0 must hold one finite entry per column of X" % who)
    return sv, Xf, b0


def logistic(f_name_ascii_Mt, dims, status, X, beta0=None, firth=2, tol=1e-10, max_iter=50, availmemGb=8, device=0):
    """eagle_logistic -> (stat fp64 (L, 4) = (gamma, se, score, log-likelihood), info int32 (L, 2) = (code, evaluations)): the logistic
    fit of status (1 / 0; -1 = not used) on the columns of X (n, c <= 15; the caller supplies the intercept) and every marker of
    Mt.ascii in turn (dims = (n, L) of M; g = 0, 1, 2 copies of the '2' character), by the rule of include/eagle_hip.h section
    1b''''iv: Newton from (beta0, 0), firth = 0 ML / 1 Firth / 2 Firth where ML fails.  beta0 = the covariates-only fit
    (r_api.logistic_null_host when None).  Codes: 0 converged, 1 max_iter, 2 singular, 3 separation, + 256 the Firth fit.  With a
    view alias status and X hold one entry per kept individual.  r_api.logistic_host restates it."""
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    sv, Xf, b0 = _logistic_inputs("logistic", n, status, X, beta0, firth, tol, max_iter)
    if b0 is None:
        from . import r_api
        b0 = np.ascontiguousarray(r_api.logistic_null_host(Xf[sv >= 0], sv[sv >= 0]))
    L = _lib.load()
    stat, info = np.zeros((nm, 4), dtype=np.float64), np.zeros((nm, 2), dtype=np.int32)
    _args_first(L.eagle_logistic, device, (os.fsencode(f_name_ascii_Mt), _dims(dims), sv.ctypes.data_as(_c_i32p), _dp(Xf), Xf.shape[1], _dp(b0),
                                           int(firth), float(tol), int(max_iter), float(availmemGb), _dp(stat), info.ctypes.data_as(_c_i32p)))
    return stat, info


# ---- admixture: EM steps of the ancestry model (include/eagle_hip.h section 1b''''v); the driver is r_api.Admixture ----
ADMIX_EPS, ADMIX_KMAX = 1e-6, 16


def _admixture_inputs(who, n, nm, Q, F, steps):
    """(Q fp64 (n, K), F fp64 (L, K), both C-ordered copies) after the checks eagle_admixture_em makes, as ValueError."""
    Qa, Fa = np.asarray(Q), np.asarray(F)
    if Qa.dtype.kind not in "iuf" or Qa.ndim != 2 or Qa.shape[0] != n or not 1 <= Qa.shape[1] <= ADMIX_KMAX:
        raise ValueError("%s: Q must be numeric (%d, K) with 1 <= K <= %d" % (who, n, ADMIX_KMAX))
    K = Qa.shape[1]
    if Fa.dtype.kind not in "iuf" or Fa.shape != (nm, K):
        raise ValueError("%s: F must be numeric (%d, %d): one row per marker, one column per column of Q" % (who, nm, K))
    if isinstance(steps, bool) or int(steps) != steps or not 0 <= steps <= 10000:
        raise ValueError("%s: steps must be a whole number in [0, 10000]" % who)
    Qf, Ff = np.array(Qa, dtype=np.float64, order="C"), np.array(Fa, dtype=np.float64, order="C")
    if not np.all(np.isfinite(Qf)) or not np.all(np.isfinite(Ff)):
        raise ValueError("%s: Q and F must be finite" % who)
    if Ff.size and (Ff.min() < ADMIX_EPS or Ff.max() > 1.0 - ADMIX_EPS):
        raise ValueError("%s: F must lie in [%g, 1 - %g]" % (who, ADMIX_EPS, ADMIX_EPS))
    if Qf.size and Qf.min() < 0.0:
        raise ValueError("%s: Q must not be negative" % who)
    rows = np.zeros(n)
    for k in range(K):                                   # the library's order of the sum
        rows = rows + Qf[:, k]
    if np.any(np.abs(rows - 1.0) > 1e-9):
        raise ValueError("%s: every row of Q must sum to 1 within 1e-9" % who)
    return Qf, Ff


def admixture_em(f_name_ascii_Mt, dims, Q, F, steps=1, availmemGb=8, device=0):
    """eagle_admixture_em -> (Q fp64 (n, K), F fp64 (L, K), loglik fp64 (steps + 1)): `steps` EM steps of the admixture model of
    include/eagle_hip.h section 1b''''v on Mt.ascii (dims = (n, L) of M), from the fractions Q (rows sum to 1) and the frequencies F
    (one ROW per marker, within [1e-6, 1 - 1e-6]) of the allele the '2' character stands for.  loglik[t] is the log-likelihood at the
    parameters entering step t, loglik[-1] that of the result; steps = 0 computes it alone.  The inputs are not modified.  With a view
    alias Q holds one row per kept individual.  r_api.admixture_host restates it."""
    n, nm = max(int(dims[0]), 0), max(int(dims[1]), 0)
    Qf, Ff = _admixture_inputs("admixture_em", n, nm, Q, F, steps)
    L = _lib.load()
    ll = np.zeros(int(steps) + 1, dtype=np.float64)
    _args_first(L.eagle_admixture_em, device, (os.fsencode(f_name_ascii_Mt), _dims(dims), Qf.shape[1], int(steps), _dp(Qf), _dp(Ff),
                                               float(availmemGb), _dp(ll)))
    return Qf, Ff, ll


# ---- the dense model algebra on the device, through the C ABI (opt-in; include/eagle_hip.h section 1c) ----
def _square_any_order(A):
    """(buffer, transposed): a float64 n x n array usable as a column-major matrix without a copy when it is contiguous in
    either order -- a C-ordered buffer read column-major is the transpose, which the callers below undo for free
    (symmetric input, or inv(A^T) = inv(A)^T).  A 200 MB layout change on one host core costs more than the device call.
    Triangles: eagle_sym_eig reads the LOWER and eagle_chol2inv the UPPER triangle of the column-major matrix (as R's eigen() and
    chol() do); a C-ordered array goes over as its transpose, so the OTHER triangle is read -- identical for an exactly symmetric
    matrix, different at rounding level for one that is symmetric only to rounding (pass np.asfortranarray(A) to pin R's triangle)."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("square matrix expected")
    if A.flags.f_contiguous and A.flags.aligned:
        return A, False
    if A.flags.c_contiguous and A.flags.aligned:
        return A, True
    return _f64F(A), False


def sym_eig(A, only_values=False, device=0):
    """eigen(A, symmetric=TRUE): (values in decreasing order, vectors in columns) like R."""
    L = _lib.load()
    ctx = context(device)
    A, _ = _square_any_order(A)   # symmetric: the transpose is the same matrix
    n = A.shape[0]
    w = np.empty(n)
    U = None if only_values else np.empty((n, n), order="F")
    _check(ctx, L.eagle_sym_eig(ctx, _dp(A), n, _dp(w), None if only_values else _dp(U)))
    return w, U


def chol2inv(A, device=0):
    """chol2inv(chol(A)); raises EagleError(1, R's chol() message) when A is not positive definite."""
    L = _lib.load()
    ctx = context(device)
    A, tr = _square_any_order(A)  # symmetric in, symmetric out: returned in the caller's order
    n = A.shape[0]
    out = np.empty((n, n), order="C" if tr else "F")
    _check(ctx, L.eagle_chol2inv(ctx, _dp(A), n, _dp(out)))
    return out


def inverse(A, device=0):
    """solve(A)."""
    L = _lib.load()
    ctx = context(device)
    A, tr = _square_any_order(A)  # a C-ordered A is handed over as A^T; inv(A^T) read back row-major is inv(A)
    n = A.shape[0]
    out = np.empty((n, n), order="C" if tr else "F")
    _check(ctx, L.eagle_inverse(ctx, _dp(A), n, _dp(out)))
    return out


def matmul(A, B, device=0):
    """A %*% B on the library's fp64 MFMA GEMM."""
    L = _lib.load()
    ctx = context(device)
    A, B = np.atleast_2d(np.asarray(A, dtype=np.float64)), np.atleast_2d(np.asarray(B, dtype=np.float64))
    m, k = A.shape
    k2, n = B.shape
    if k != k2:
        raise ValueError("non-conformable arguments")
    if A.flags.c_contiguous and B.flags.c_contiguous and A.flags.aligned and B.flags.aligned and not (A.flags.f_contiguous and B.flags.f_contiguous):
        # row-major operands: their buffers read column-major are A^T (k x m) and B^T (n x k); B^T A^T = (A B)^T, whose
        # column-major image is A B row-major -- no layout change on the host
        out = np.empty((m, n), order="C")
        _check(ctx, L.eagle_matmul(ctx, _dp(B), _dp(A), n, k, m, _dp(out)))
        return out
    A, B = _f64F(A), _f64F(B)
    out = np.empty((m, n), order="F")
    _check(ctx, L.eagle_matmul(ctx, _dp(A), _dp(B), m, k, n, _dp(out)))
    return out


def mmt_sqrt_and_sqrtinv(MMt, device=0):
    """E/R/calculateMMt_sqrt_and_sqrtinv.R:15-47 -> (sqrt, invsqrt, trace of their product), or None where the R function
    returns NULL (MMt not positive definite)."""
    L = _lib.load()
    ctx = context(device)
    M = _f64F(MMt)
    n = M.shape[0]
    sq, inv = np.zeros((n, n), order="F"), np.zeros((n, n), order="F")
    tr = C.c_double()
    rc = _check(ctx, L.eagle_mmt_sqrt_and_sqrtinv(ctx, _dp(M), n, _dp(sq), _dp(inv), C.byref(tr)), soft_ok=True)
    if rc == 1:
        return None
    return sq, inv, tr.value


def last_error(device=0):
    return _lib.load().eagle_last_error(context(device)).decode()
