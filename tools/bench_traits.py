#!/usr/bin/env python3
"""Many traits over one Z (eagle_spectral_scan_traits).  Prints one JSON line and writes it to the path given by --out.

scan: the pass over a device-resident Z of n x L (default the headline 10,000 x 1,000,000; Z = 80 GB fp64) for T traits with
      p_t = 5 fixed-effect columns: the batched pass (eagle_dev_spectral_pass_traits, one launch per column group) against T
      single-trait passes (eagle_dev_spectral_pass, NC = 16), HIP events, one warm-up, median of 3.  Per pass the bound is
      max(8 L n_pad bytes / 8 TB/s, 2 L n_pad 16 nt flop / 78.6 TF) (datasheet peaks; nt = MFMA tiles of the group).
e2e:  AM_traits with T = 16 and maxit = 10 against 16 AM(..., backend=SpectralBackend()) runs on text files of n_e2e x L_e2e,
      split into setup (calcMMt, eigh, Z build), scans (spectral_scan_traits + spectral_rows) and host algebra (the rest).
Usage: tools/bench_traits.py [--n N] [--L L] [--n-e2e N] [--L-e2e L] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F64_MFMA = 78.6e12
PEAK_HBM = 8.0e12


def pad(x):
    return (x + 255) // 256 * 256


def groups_for(T, p):
    """spectral_trait_groups (csrc/eagle_host.h) for T traits of p columns: [(traits, ntl, nt)]."""
    out, t0, lin = [], 0, 0
    for t in range(T):
        if t > t0 and (lin + p + 1 + 15) // 16 + (t - t0 + 1 + 15) // 16 > 8:
            out.append((t - t0, (lin + 15) // 16, (lin + 15) // 16 + (t - t0 + 15) // 16))
            t0, lin = t, p + 1
        else:
            lin += p + 1
    out.append((T - t0, (lin + 15) // 16, (lin + 15) // 16 + (T - t0 + 15) // 16))
    return out


def bench_scan(n, L, Ts, p=5):
    import torch
    from eagleeverything_amd import _lib, rcpp_api
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    dev = torch.device("cuda:0")
    np_, Lp = pad(n), pad(L)
    Z = torch.empty((Lp, np_), dtype=torch.float64, device=dev)
    for r in range(0, Lp, 65536):
        Z[r:r + 65536].normal_()
    Z[:, n:] = 0
    G16 = torch.randn((np_, 16), dtype=torch.float64, device=dev)
    d = torch.rand(np_, dtype=torch.float64, device=dev) + 0.5
    lin = torch.empty((Lp, 16), dtype=torch.float64, device=dev)
    quad = torch.empty(Lp, dtype=torch.float64, device=dev)
    Gb = torch.randn((np_, 128), dtype=torch.float64, device=dev)
    out = torch.empty((Lp, 128), dtype=torch.float64, device=dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())

    def single():
        assert lib.eagle_dev_spectral_pass(ctx, vp(Z), Lp, np_, vp(G16), 16, vp(d), vp(lin), vp(quad), stream()) == 0

    def batched(gr):
        for _, ntl, nt in gr:
            assert lib.eagle_dev_spectral_pass_traits(ctx, vp(Z), Lp, np_, vp(Gb), nt, ntl, vp(out), stream()) == 0

    def timed(fn, reps=3):
        fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    one_ms = timed(single)
    res = {"n": n, "L": L, "p": p, "single_pass_ms": one_ms, "rows": []}
    for T in Ts:
        gr = groups_for(T, p)
        b_ms = timed(lambda: batched(gr))
        s_ms = timed(lambda: [single() for _ in range(T)])
        floor_s = sum(max(8.0 * Lp * np_ / PEAK_HBM, 2.0 * Lp * np_ * 16 * nt / PEAK_F64_MFMA) for _, _, nt in gr)
        binds = ["HBM" if 8.0 / PEAK_HBM >= 2.0 * 16 * nt / PEAK_F64_MFMA else "fp64 MFMA" for _, _, nt in gr]
        res["rows"].append({"T": T, "passes": len(gr), "tiles": [nt for _, _, nt in gr], "batched_ms": b_ms, "sequential_ms": s_ms,
                            "speedup": s_ms / b_ms, "bound_ms": floor_s * 1e3, "fraction_of_bound": floor_s * 1e3 / b_ms,
                            "bound_by": sorted(set(binds))})
    del Z, out, Gb
    torch.cuda.empty_cache()
    return res


def bench_e2e(n, L, T=16, maxit=10):
    from eagleeverything_amd import am, r_api, rcpp_api, synth
    Mt8 = synth.genotypes_marker_major(n, L, seed=11)
    rng = np.random.default_rng(3)
    Y = np.column_stack([synth.trait(Mt8, nqtl=3 + t % 4, beta=0.6, seed=100 + t)[0] for t in range(T)])
    X = np.column_stack([np.ones(n), rng.standard_normal(n)])
    clock = {"scan": 0.0}
    orig = {k: getattr(rcpp_api, k) for k in ("spectral_prepare", "spectral_scan_traits", "spectral_rows")}

    def timed(name):
        def f(*a, **kw):
            t = time.perf_counter()
            r = orig[name](*a, **kw)
            if name == "spectral_prepare":
                clock["setup_end"] = time.perf_counter()
            else:
                clock["scan"] += time.perf_counter() - t
            return r
        return f

    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as dname:
        geno = synth.write_geno_pair(dname, Mt8)
        am.AM(Y[:, 0], X, geno, maxit=2, backend=am.SpectralBackend())      # warm-up: code objects, resident files
        for k in orig:
            setattr(rcpp_api, k, timed(k))
        t0 = time.perf_counter()
        res = am.AM_traits(Y, X, geno, maxit=maxit)
        total = time.perf_counter() - t0
        for k, v in orig.items():
            setattr(rcpp_api, k, v)
        setup = clock["setup_end"] - t0
        t1 = time.perf_counter()
        refs = [am.AM(Y[:, t], X, geno, maxit=maxit, backend=am.SpectralBackend()) for t in range(T)]
        seq = time.perf_counter() - t1
        same = all(r["all_picks"] == q["all_picks"] for r, q in zip(res, refs))
        rcpp_api.drop_cache()
    return {"n": n, "L": L, "T": T, "maxit": maxit, "am_traits_s": total, "setup_s": setup, "scans_s": clock["scan"],
            "host_algebra_s": total - setup - clock["scan"], "sequential_am_spectral_s": seq, "speedup": seq / total,
            "same_picks": same, "picks_per_trait": [len(r["all_picks"]) for r in res]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--L", type=int, default=1000000)
    ap.add_argument("--n-e2e", type=int, default=1000)
    ap.add_argument("--L-e2e", type=int, default=50000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"scan": bench_scan(a.n, a.L, (1, 4, 16, 64)), "e2e": bench_e2e(a.n_e2e, a.L_e2e)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
