"""Times the exact per-marker mixed-model test (include/eagle_hip.h section 1d') beside the scan it refines, on ONE resident Z = Mt U of
a synthetic panel (default n x L = 2,048 x 32,768), in one run:

    spectral_scan_c<c>_ms    eagle_spectral_scan with c = 1, 4, 14 fixed-effect columns: the P3D score test, the HBM-bound yardstick
    lmm_<method>_c<c>_ms     eagle_spectral_lmm, method reml / ml, the same c, tol 1e-10, max_iter 50, every marker, from the null fit's
                             ln delta: the staging of B16 and lambda, k_lmm_exact<method>, L x 5 fp64 and L x 2 int32 to the host

The genotypes are synth's, the covariates standard normal, the trait has a polygenic part on every marker, four planted markers and
noise in the proportion that keeps the null fit's delta inside the limits.  K, its eigh and
spectral_prepare run once and are not timed.  The calls are alternated rep by rep, medians reported with min and max, and with them the
mean number of evaluations per marker (iterations + 1) and the count of every code.  Before timing, the head of each result is compared
with r_api.lmm_host on the device's own rows of Z (equal codes, |gamma| within 1e-8).  Wall-clock times of WHOLE calls; no kernel is
timed on its own (a kernel trace is a run of its own).

    python tools/lmm_timing.py [n] [L] [reps] [out.json]      (default 2048 32768 5 profiles/r20_lmm.json)
"""
import json
import math
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CS = (1, 4, 14)


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 2048, int), arg(2, 32768, int), arg(3, 5, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r20_lmm.json"), str)
    import torch
    from epistasis_timing import alternate
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    out = {"reps": reps, "device": torch.cuda.get_device_name(0), "n": n, "L": L, "tol": 1e-10, "max_iter": 50, "z_bytes": 8 * L * n,
           "what": "wall-clock times of whole calls on a resident Z (host staging and transfers included), the calls alternated, medians",
           "not_timed": "the kernel on its own, an index list (p_exact), K / eigh / spectral_prepare, other sizes, 10,000 x 1,000,000"}
    head = 48
    Mt8 = synth.genotypes_marker_major(n, L, seed=20)
    rng = np.random.default_rng(20)
    qtl = rng.choice(L, 4, replace=False)
    # a polygenic part on every marker (variance 3.3) under noise of variance 2.25: the null fit's delta lies inside the limits
    poly = np.zeros(n)
    for r0 in range(0, L, 4096):
        poly += Mt8[r0:r0 + 4096].astype(np.float32).T.astype(np.float64) @ rng.standard_normal(min(4096, L - r0))
    y = Mt8[qtl].astype(np.float64).T @ [0.5, -0.4, 0.3, 0.3] + math.sqrt(3.3 / (0.6 * L)) * poly + 1.5 * rng.standard_normal(n)
    with tempfile.TemporaryDirectory() as d:
        geno = synth.write_geno_pair(d, Mt8)
        be = am.SpectralBackend()
        be.calcMMt(geno, 8, 1, np.array([np.nan]), True)
        lam, U = be.eig
        Uty = U.T @ y
        Zh = rcpp_api.spectral_rows(np.arange(head)).T
        ops = {}
        for c in CS:
            X = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])
            UtX = U.T @ X
            fit = {"reml": am.emma_REMLE_eig(lam, UtX, Uty), "ml": am.emma_MLE_eig(lam, UtX, Uty)}
            ops[c] = (UtX, fit)
            for m in ("reml", "ml"):
                th = math.log(fit[m]["delta"])
                stat, info = rcpp_api.spectral_lmm(lam, UtX, Uty, reml=m == "reml", theta0=th, n_markers=L)
                hs, hi = r_api.lmm_host(lam, UtX, Uty, Zh, reml=m == "reml", theta0=th)
                assert np.array_equal(info[:head, 0], hi[:, 0]), "eagle_spectral_lmm's codes differ from lmm_host at c = %d" % c
                ok = hi[:, 0] != 2
                assert np.all(np.abs(stat[:head][ok, 0] - hs[ok, 0]) <= 1e-8), "eagle_spectral_lmm differs from lmm_host at c = %d" % c
                key = "lmm_%s_c%d" % (m, c)
                out[key + "_theta0"] = th
                out[key + "_mean_evaluations"] = float(info[:, 1].mean() + 1.0)
                out[key + "_max_evaluations"] = int(info[:, 1].max() + 1)
                out[key + "_codes"] = [int(v) for v in np.bincount(info[:, 0], minlength=5)]
        fns, names = [], []
        for c in CS:
            UtX, fit = ops[c]
            fns.append(lambda UtX=UtX, fit=fit: rcpp_api.spectral_scan(lam, UtX, Uty, fit["reml"]["ve"], fit["reml"]["vg"], L))
            names.append("spectral_scan_c%d" % c)
            for m in ("reml", "ml"):
                fns.append(lambda UtX=UtX, fit=fit, m=m: rcpp_api.spectral_lmm(lam, UtX, Uty, reml=m == "reml", theta0=math.log(fit[m]["delta"]),
                                                                              n_markers=L))
                names.append("lmm_%s_c%d" % (m, c))
        for name, t in zip(names, alternate(torch, fns, reps)):
            out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
        for c in CS:
            for m in ("reml", "ml"):
                key = "lmm_%s_c%d" % (m, c)
                out[key + "_over_spectral_scan"] = out[key + "_ms"] / out["spectral_scan_c%d_ms" % c]
                out[key + "_ns_per_marker_individual_evaluation"] = out[key + "_ms"] * 1e6 / (L * float(n) * out[key + "_mean_evaluations"])
        rcpp_api.drop_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
