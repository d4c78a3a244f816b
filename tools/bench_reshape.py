#!/usr/bin/env python3
"""AM() with missing trait records: eagle_reshape_m in FILES mode against VIEW mode (include/eagle_hip.h).  Prints one JSON line:
  files_s ............ FILES-mode wall time (the reference's rewrite of M.ascii and Mt.ascii), n x L_files text
  view_first_s ....... registering the views + the first MM^T + scan on them, Mt read from its 2-bit sidecar, n x L_files
  gather_ms, gather_TBps   k_gather_cols_i8 alone (HIP events, median of 5) on a resident n x L image, n x L (default the
                       headline 10,000 x 1,000,000): read L*ld_src + write L*ld_out bytes; judged against 4.5 TB/s
  scan_view_s / scan_files_s / scan_ratio   steady-state scan step (calculate_a_and_vara, resident) on the view and on the
                       rewritten file, median of 5: the kernels and n are the same, so the ratio must be within 2 %
File- and PCIe-inclusive timings: never bench.py's value.
Usage: tools/bench_reshape.py [n] [L] [L_files] [NA fraction]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
    L_files = int(sys.argv[3]) if len(sys.argv) > 3 else L
    frac = float(sys.argv[4]) if len(sys.argv) > 4 else 0.01
    import ctypes as C

    import torch
    from eagleeverything_amd import _lib, rcpp_api, synth
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    rng = np.random.default_rng(0)
    na = np.sort(rng.choice(n, max(1, int(round(frac * n))), replace=False))
    keep = np.setdiff1d(np.arange(n), na).astype(np.int32)
    nk = keep.size
    pad = lambda x: (x + 255) // 256 * 256
    out = {"n": n, "L": L, "L_files": L_files, "n_na": int(na.size),
           "library_host_threads": min(16, os.cpu_count() or 1)}   # the library's reader / writer threads (host_threads())

    # 1. k_gather_cols_i8 alone at n x L
    dev = torch.device("cuda:0")
    src = torch.randint(-1, 2, (pad(L), pad(n)), dtype=torch.int8, device=dev)
    dst = torch.empty((pad(L), pad(nk)), dtype=torch.int8, device=dev)
    dmap = torch.from_numpy(keep).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    gather = lambda: lib.eagle_dev_gather_cols_i8(ctx, C.c_void_p(src.data_ptr()), src.shape[1], C.c_void_p(dmap.data_ptr()), 0, L, nk,
                                                  C.c_void_p(dst.data_ptr()), dst.shape[1], C.c_void_p(stream))
    assert gather() == 0
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gather()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = float(np.median(ts))
    exp = src[:L][:, torch.from_numpy(keep.astype(np.int64)).to(dev)]
    assert torch.equal(dst[:L, :nk], exp) and not dst[:L, nk:].any(), "gather differs from the indexing"
    out["gather_ms"] = ms
    out["gather_TBps"] = (L * pad(n) + L * pad(nk)) / (ms * 1e-3) / 1e12
    out["gather_target_TBps"] = 4.5
    del src, dst, exp
    torch.cuda.empty_cache()

    # 2. files of n x L_files
    Mt8 = synth.genotypes_marker_major(n, L_files, seed=7)
    A = rng.standard_normal((nk, 64)) / 8.0
    S = np.asfortranarray(np.eye(nk) + A @ A.T)
    V = np.asfortranarray(0.5 * np.eye(nk) - 0.01 * (A[:, :8] @ A[:, :8].T))
    ahat = rng.standard_normal(nk)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        df, dv = os.path.join(d, "f"), os.path.join(d, "v")
        os.mkdir(df)
        os.mkdir(dv)
        gf = synth.write_geno_pair(df, Mt8)
        fMv, fMtv = os.path.join(dv, "M.ascii"), os.path.join(dv, "Mt.ascii")
        synth.write_ascii(fMv, np.ascontiguousarray(Mt8.T))
        del Mt8
        rcpp_api.createMt_ASCII_rcpp(fMv, fMtv, "text", 8.0, (n, L_files))   # Mt.ascii + its 2-bit sidecar
        rcpp_api.drop_cache()
        t = time.perf_counter()
        nd = rcpp_api.ReshapeM_rcpp(gf["asciifileM"], gf["asciifileMt"], na, (n, L_files))
        out["files_s"] = time.perf_counter() - t
        before = rcpp_api.view_load_counts()
        t = time.perf_counter()
        nd_v = rcpp_api.ReshapeM_rcpp(fMv, fMtv, na, (n, L_files), view=True)
        rcpp_api.calculateMMt_rcpp(fMv + "tmp", 8.0, 16, np.nan, nd_v)
        rcpp_api.calculate_a_and_vara_rcpp(fMtv + "tmp", np.nan, S, V, 8.0, (L_files, nk), ahat)
        out["view_first_s"] = time.perf_counter() - t
        after = rcpp_api.view_load_counts()
        out["view_first_loads"] = {k: after[k] - before[k] for k in after}   # M from text, Mt from the sidecar
        assert nd == nd_v

        def steady(f):
            rcpp_api.calculate_a_and_vara_rcpp(f, np.nan, S, V, 8.0, (L_files, nk), ahat)
            ts = []
            for _ in range(5):
                t = time.perf_counter()
                r = rcpp_api.calculate_a_and_vara_rcpp(f, np.nan, S, V, 8.0, (L_files, nk), ahat)
                ts.append(time.perf_counter() - t)
            return float(np.median(ts)), r
        out["scan_view_s"], rv = steady(fMtv + "tmp")
        out["scan_files_s"], rf = steady(gf["asciifileMt"] + "tmp")
        out["scan_ratio"] = out["scan_view_s"] / out["scan_files_s"]
        out["scan_bit_equal"] = bool(np.array_equal(rv["a"], rf["a"]) and np.array_equal(rv["vara"], rf["vara"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
