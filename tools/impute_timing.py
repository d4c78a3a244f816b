"""Times kNN imputation (include/eagle_hip.h section 1b'''i) on ONE synthetic .bed file in one run:

  counts_ms            eagle_bed_marker_counts: the yardstick (pread of the windows into pinned memory, copy to the device,
                       k_bed_marker_counts, L x 4 int32 to the host)
  impute_ms            eagle_bed_impute_knn on the same file, page cache warm: the same staging, k_bed_marker_counts AND k_bed_impute
                       per window, the patched windows copied back and written to a new file, the n x K table uploaded once
  impute_over_counts   their ratio: what the imputation kernel and the write-back add to a pass over the file
  knn_rows_ms          eagle_knn_rows alone on random n x n int32 matrices of the value range of L markers (host arrays in and out:
                       two n x n uploads, n blocks of k_knn_rows, n x K back)

The two .bed calls are alternated rep by rep, medians reported.  Before timing, the first 256 markers of the output are compared with
r_api.impute_knn_host and the counts' row sums with the missing column of eagle_bed_marker_counts.  Wall-clock times of whole calls,
host transfers and file I/O included; no kernel is timed on its own.

    python tools/impute_timing.py [n] [L] [reps] [out.json] [missing rate] [K] [k]
                                                               (default 4096 65536 7 profiles/r10_impute.json 0.05 64 10)
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 4096, int), arg(2, 65536, int), arg(3, 7, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r10_impute.json"), str)
    rate, K, k = arg(5, 0.05, float), arg(6, 64, int), arg(7, 10, int)
    import torch
    from eagleeverything_amd import r_api, rcpp_api
    rng = np.random.default_rng(0)
    # random matrices with the shape of eagle_sample_ibs' results: symmetric, ibs0 zero on the diagonal
    ibs0 = rng.integers(0, max(L // 4, 1), size=(n, n), dtype=np.int32)
    ibs0 = np.triu(ibs0, 1) + np.triu(ibs0, 1).T
    hethet = rng.integers(0, max(L // 4, 1), size=(n, n), dtype=np.int32)
    hethet = np.triu(hethet, 1) + np.triu(hethet, 1).T + np.diag(rng.integers(L // 4, max(L // 2, 2), size=n)).astype(np.int32)
    nbr = rcpp_api.knn_rows(ibs0, hethet, K)
    head = min(n, 256)
    assert np.array_equal(nbr[:head], r_api.knn_rows_host(r_api.knn_distance(ibs0, hethet), K)[:head]), "knn_rows differs from numpy"
    t_knn = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rcpp_api.knn_rows(ibs0, hethet, K)
        t_knn.append((time.perf_counter() - t0) * 1e3)
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "panel")
        rb = (n + 3) // 4
        with open(prefix + ".bed", "wb") as f:                       # random codes, `rate` of them the missing code, in bands of markers
            f.write(b"\x6c\x1b\x01")
            lut = np.array([0, 2, 3], dtype=np.uint8)
            for r0 in range(0, L, 4096):
                c = lut[rng.integers(0, 3, size=(min(4096, L - r0), n))]
                c[rng.random(c.shape) < rate] = 1
                f.write(r_api.pack_bed_codes(c).tobytes())
        bed, out_bed, dims = prefix + ".bed", os.path.join(d, "imputed.bed"), (n, L)
        f_cnt = lambda: rcpp_api.bed_marker_counts(bed, dims)
        f_imp = lambda: rcpp_api.bed_impute_knn(bed, dims, nbr, k, 1, out_bed)
        mc = f_cnt()                                                  # warm-up: page cache, staging buffers
        counts = f_imp()
        assert np.array_equal(counts.sum(axis=1), mc[:, 3]), "imputed genotypes are not the missing ones"
        Lh = min(L, 256)
        raw = np.fromfile(bed, dtype=np.uint8, count=3 + Lh * rb)[3:].reshape(Lh, rb)
        codes = np.stack([(raw >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(Lh, 4 * rb)[:, :n]
        rows, want = r_api.impute_knn_host(codes, nbr, k, 1)
        got = np.fromfile(out_bed, dtype=np.uint8, count=3 + Lh * rb)
        assert bytes(got[:3]) == b"\x6c\x1b\x01" and np.array_equal(got[3:].reshape(Lh, rb), rows), "k_bed_impute differs from numpy"
        assert np.array_equal(counts[:Lh], want)
        fns = [f_cnt, f_imp]
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
    out = {"n": n, "L": L, "reps": reps, "missing_rate": rate, "K": K, "k": k, "bed_bytes": 3 + L * rb,
           "n_missing": int(mc[:, 3].sum(dtype=np.int64)), "by_vote": int(counts[:, 0].sum(dtype=np.int64)),
           "by_fallback": int(counts[:, 1].sum(dtype=np.int64)), "device": torch.cuda.get_device_name(0),
           "what": "wall-clock times of whole calls (file I/O from a warm page cache and host transfers included), the two .bed calls "
                   "alternated, medians; random genotypes, random symmetric matrices for knn_rows",
           "not_timed": "the kernels on their own, the cold-cache file, a file of several staging windows, ImputeBed as a whole "
                        "(its eagle_sample_ibs and second ingestion)"}
    for name, t in zip(("counts", "impute", "knn_rows"), ts + [t_knn]):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    out["impute_over_counts"] = out["impute_ms"] / out["counts_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
