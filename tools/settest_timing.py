"""Times the set test (include/eagle_hip.h section 1d'') beside the scan whose scores it shares, on ONE resident Z = Mt U of a synthetic
panel (default n x L = 2,048 x 32,768, the panel of tools/lmm_timing.py), in one run:

    spectral_scan_c<c>_ms      eagle_spectral_scan with c = 1, 14 fixed-effect columns: one pass over Z, the HBM-bound yardstick
    settest_m<m>_c<c>_ms       eagle_spectral_settest on non-overlapping windows of m = 16, 64 markers that cover all L markers, weights 1,
                               the same c: the staging of the operand image, d and the CSR lists, k_settest_gram, 7 fp64 and 2 int32 per set
                               to the host (no score_out, no cov_out)
    settest_m<m>_c<c>_cov_ms   the same call with score_out and cov_out (m^2 fp64 per set more to the host)

The library is called through ctypes on CSR arrays made once, so the Python wrapper's list handling is not in the figures.  K, its eigh
and spectral_prepare run once and are not timed.  The calls are alternated rep by rep, medians reported with min and max.  Before
timing, the first sets of each result are compared with r_api.settest_host on the device's own rows of Z (equal codes, the seven
statistics within 1e-9 relative).  Wall-clock times of WHOLE calls; no kernel is timed on its own (a kernel trace is a run of its own).

    python tools/settest_timing.py [n] [L] [reps] [out.json]      (default 2048 32768 5 profiles/r22_settest.json)
"""
import ctypes as C
import json
import math
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CS = (1, 14)
MS = (16, 64)


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 2048, int), arg(2, 32768, int), arg(3, 5, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r22_settest.json"), str)
    import torch
    from epistasis_timing import alternate
    from eagleeverything_amd import _lib, am, r_api, rcpp_api, synth
    from eagleeverything_amd._lib import c_dp, c_lp
    out = {"reps": reps, "device": torch.cuda.get_device_name(0), "n": n, "L": L, "z_bytes": 8 * L * n,
           "what": "wall-clock times of whole calls on a resident Z (host staging and transfers included), the calls alternated, medians",
           "not_timed": "the kernel on its own, counters, overlapping or ragged sets, weights, K / eigh / spectral_prepare, other sizes"}
    Mt8 = synth.genotypes_marker_major(n, L, seed=20)
    rng = np.random.default_rng(20)
    qtl = rng.choice(L, 4, replace=False)
    poly = np.zeros(n)
    for r0 in range(0, L, 4096):
        poly += Mt8[r0:r0 + 4096].astype(np.float32).T.astype(np.float64) @ rng.standard_normal(min(4096, L - r0))
    y = Mt8[qtl].astype(np.float64).T @ [0.5, -0.4, 0.3, 0.3] + math.sqrt(3.3 / (0.6 * L)) * poly + 1.5 * rng.standard_normal(n)
    lib = _lib.load()
    dp = lambda a: a.ctypes.data_as(c_dp)
    lp = lambda a: a.ctypes.data_as(c_lp)
    with tempfile.TemporaryDirectory() as d:
        geno = synth.write_geno_pair(d, Mt8)
        be = am.SpectralBackend()
        be.calcMMt(geno, 8, 1, np.array([np.nan]), True)
        ctx = rcpp_api.context(0)
        lam, U = be.eig
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        Uty = np.ascontiguousarray(U.T @ y)
        head = 4
        fns, names, keep = [], [], []
        for c in CS:
            X = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])
            UtX = np.asfortranarray(U.T @ X)
            fit = am.emma_REMLE_eig(lam, UtX, Uty)
            ve, vg = float(fit["ve"]), float(fit["vg"])
            fns.append(lambda UtX=UtX, ve=ve, vg=vg: rcpp_api.spectral_scan(lam, UtX, Uty, ve, vg, L))
            names.append("spectral_scan_c%d" % c)
            for m in MS:
                sets = r_api.sets_from_windows(L, size=m)["sets"]
                ptr, idx, w = rcpp_api.settest_csr(sets)
                k = len(sets)
                stat, info = np.zeros((k, 7)), np.zeros((k, 2), dtype=np.int32)
                score, cov = np.zeros(idx.size), np.zeros(int(np.sum(np.diff(ptr) ** 2)))
                keep.append((UtX, ptr, idx, w, stat, info, score, cov))

                def call(full, UtX=UtX, ve=ve, vg=vg, c=c, k=k, ptr=ptr, idx=idx, w=w, stat=stat, info=info, score=score, cov=cov):
                    rc = lib.eagle_spectral_settest(ctx, dp(lam), dp(UtX), dp(Uty), c, ve, vg, k, lp(ptr), lp(idx), dp(w), dp(stat),
                                                    info.ctypes.data_as(C.POINTER(C.c_int32)), dp(score) if full else None, dp(cov) if full else None)
                    assert rc == 0, lib.eagle_last_error(ctx).decode()

                call(True)
                Zh = rcpp_api.spectral_rows(np.arange(head * m)).T
                host = r_api.settest_host(lam, UtX, Uty, Zh, ve, vg, sets[:head])
                assert np.array_equal(info[:head], host["info"]), "eagle_spectral_settest's codes differ from settest_host at m = %d, c = %d" % (m, c)
                assert np.allclose(stat[:head], host["stat"], rtol=1e-9, atol=0.0), "eagle_spectral_settest differs from settest_host"
                key = "settest_m%d_c%d" % (m, c)
                out[key + "_sets"] = k
                out[key + "_codes"] = [int(v) for v in np.bincount(info[:, 0], minlength=3)]
                fns += [lambda call=call: call(False), lambda call=call: call(True)]
                names += [key, key + "_cov"]
        for name, t in zip(names, alternate(torch, fns, reps)):
            out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
        for c in CS:
            for m in MS:
                key = "settest_m%d_c%d" % (m, c)
                out[key + "_over_spectral_scan"] = out[key + "_ms"] / out["spectral_scan_c%d_ms" % c]
                out[key + "_z_tb_per_s"] = 8.0 * L * n / (out[key + "_ms"] * 1e-3) / 1e12
        rcpp_api.drop_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
