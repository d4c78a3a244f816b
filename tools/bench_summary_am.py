#!/usr/bin/env python3
"""SummaryAM after AM(..., SpectralBackend()).  Prints one JSON line and writes it to the path given by --out.

eigen: r_api.SummaryAM on text files of n x L after AM(..., backend=SpectralBackend(), algebra="device") picked k markers:
       with eig=backend.eig (no eigh), and with one fresh eigh of K on the device (algebra="device").  Best of --reps runs each,
       one warm-up; calcMMt and the device eigh of K are also timed on their own.
straight: summary_am.R:142-211 restated with n x n algebra (solve(H), emma.REMLE / emma.MLE with their eigen() calls, the
       yardstick of tests/test_summary_am_host.py) on the same picks at n_straight x L_straight, against SummaryAM there.
Usage: tools/bench_summary_am.py [--n N] [--L L] [--maxit K] [--n-straight N] [--L-straight L] [--reps R] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def straight_summary(y, baseX, Msel, K):
    from scipy.stats import chi2
    from eagleeverything_amd import am
    n, q = baseX.shape
    F = np.column_stack([baseX, Msel])
    eR = am.emma_REMLE(y, F, K, llim=-100, ulim=100)
    Hinv = np.linalg.solve(eR["vg"] * K + eR["ve"] * np.eye(n), np.eye(n))
    Ainv = np.linalg.solve(F.T @ Hinv @ F, np.eye(F.shape[1]))
    beta = Ainv @ F.T @ Hinv @ y
    W = beta ** 2 / np.diag(Ainv)
    K2 = K / K.max() + 0.05 * np.eye(n)
    base = am.emma_MLE(y, baseX, K2, llim=-100, ulim=100)["ML"]
    rsq = [1 - math.exp(-2 / n * (am.emma_MLE(y, F[:, :q + k], K2, llim=-100, ulim=100)["ML"] - base))
           for k in range(1, Msel.shape[1] + 1)]
    return beta, W, 1 - chi2.cdf(W, 1), np.array(rsq)


def am_run(n, L, maxit, dname, seed):
    from eagleeverything_amd import am, host_model, synth
    Mt8 = synth.genotypes_marker_major(n, L, seed=seed)
    y, _ = synth.trait(Mt8, nqtl=maxit + 4, beta=0.3, seed=seed + 1)
    X = np.column_stack([np.ones(n), np.random.default_rng(seed).standard_normal(n)])
    geno = synth.write_geno_pair(dname, Mt8)
    spec = am.SpectralBackend()
    t = time.perf_counter()
    try:
        res = am.AM(y, X, geno, maxit=maxit, backend=spec, algebra="device")
    finally:
        host_model.set_algebra("host")
    return Mt8, y, X, geno, spec, res, time.perf_counter() - t


def timed(fn, reps):
    best, out = float("inf"), None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t)
    return best, out


def bench_eigen(n, L, maxit, reps):
    from eagleeverything_amd import host_model, r_api, rcpp_api
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as dname:
        Mt8, y, X, geno, spec, res, t_am = am_run(n, L, maxit, dname, seed=31)
        r_api.SummaryAM(res, y, X, geno, eig=spec.eig)                       # warm-up
        t_eig, s_eig = timed(lambda: r_api.SummaryAM(res, y, X, geno, eig=spec.eig), reps)
        host_model.set_algebra("device")
        try:
            t_dev, s_dev = timed(lambda: r_api.SummaryAM(res, y, X, geno), reps)
            t = time.perf_counter()
            K = r_api.calcMMt(geno, 8, 1, np.array([np.nan]), True)
            t_k = time.perf_counter() - t
            t = time.perf_counter()
            host_model.algebra().eigh(K)
            t_e = time.perf_counter() - t
        finally:
            host_model.set_algebra("host")
        rel = max(float(np.max(np.abs(np.subtract(s_eig[p][k], s_dev[p][k])) / np.abs(s_dev[p][k])))
                  for p, k in (("size", "estimate"), ("pvalue", "W"), ("R", "Prop_var_explained")))
        rcpp_api.drop_cache()
    return {"n": n, "L": L, "k": len(res["selected_loci"]), "am_spectral_s": t_am, "summary_eig_reused_s": t_eig,
            "summary_fresh_device_eigh_s": t_dev, "calcMMt_s": t_k, "device_eigh_s": t_e, "max_rel_diff_reused_vs_fresh": rel}


def bench_straight(n, L, maxit):
    from eagleeverything_amd import r_api, rcpp_api
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as dname:
        Mt8, y, X, geno, spec, res, _ = am_run(n, L, maxit, dname, seed=41)
        t_eig, s = timed(lambda: r_api.SummaryAM(res, y, X, geno, eig=spec.eig), 1)
        t_fresh, _ = timed(lambda: r_api.SummaryAM(res, y, X, geno), 1)
        K = r_api.calcMMt(geno, 8, 1, np.array([np.nan]), True)
        Msel = Mt8[np.array(res["selected_loci"]) - 1].T.astype(np.float64)
        t = time.perf_counter()
        beta, W, _, rsq = straight_summary(y, X, Msel, K)
        t_straight = time.perf_counter() - t
        rel = max(float(np.max(np.abs(np.asarray(s[p][k]) - r) / np.abs(r)))
                  for (p, k), r in ((("size", "estimate"), beta), (("pvalue", "W"), W), (("R", "Prop_var_explained"), rsq)))
        rcpp_api.drop_cache()
    return {"n": n, "L": L, "k": len(res["selected_loci"]), "straight_s": t_straight, "summary_eig_reused_s": t_eig,
            "summary_fresh_host_eigh_s": t_fresh, "speedup_fresh": t_straight / t_fresh, "max_rel_diff_vs_straight": rel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--L", type=int, default=100000)
    ap.add_argument("--maxit", type=int, default=15)
    ap.add_argument("--n-straight", type=int, default=2000)
    ap.add_argument("--L-straight", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"eigen": bench_eigen(a.n, a.L, a.maxit, a.reps)}
    print("eigen:", json.dumps(out["eigen"]), file=sys.stderr, flush=True)
    out["straight"] = bench_straight(a.n_straight, a.L_straight, a.maxit)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
