"""Times the sample-QC entry points of include/eagle_hip.h section 1b''' on ONE resident synthetic M.ascii in one run:

  mmt_ms               eagle_calculateMMt: the yardstick (one fp4 SYRK on the cached operand image, finish, n x n fp64 to the host)
  ibs_ms               eagle_sample_ibs on the same resident file (the same SYRK for D, k_f4_abs + a second SYRK for Q, k_ibs_finish,
                       two n x n int32 matrices to the host: the same bytes over PCIe)
  ibs_over_mmt         their ratio; from the code about 2 is expected
  sample_counts_ms     eagle_sample_counts (k_marker_counts on the individual-major image, one HBM-bound read)
  hwe_ms               eagle_hwe_exact alone, on L2 = 1,000,000 markers of N individuals drawn near Hardy-Weinberg proportions, host
                       arrays in and out; hwe_markers_per_s from it

The two Gram calls are alternated rep by rep, medians reported; both results are checked against each other first (D = Q - 2 ibs0
must be the MM^T the yardstick returns).  Wall-clock times of whole calls, host transfers included.

    python tools/sample_qc_timing.py [n] [L] [reps] [out.json]      (default 4096 65536 7 profiles/r08_sample_qc.json)
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
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "r08_sample_qc.json")
    import torch
    from eagleeverything_amd import rcpp_api, synth
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        fM = os.path.join(d, "M.ascii")
        block = 256
        with open(fM, "wb") as f:                                   # n lines of L characters, written in bands of individuals
            for r0 in range(0, n, block):
                g = rng.integers(0, 3, size=(min(block, n - r0), L), dtype=np.uint8) + ord("0")
                f.write(np.concatenate([g, np.full((g.shape[0], 1), ord("\n"), dtype=np.uint8)], axis=1).tobytes())
        dims = (n, L)
        f_mmt = lambda: rcpp_api.calculateMMt_rcpp(fM, 8.0, 16, np.nan, dims)
        f_ibs = lambda: rcpp_api.sample_ibs(fM, dims)
        f_cnt = lambda: rcpp_api.sample_counts(fM, dims)
        mmt = f_mmt()                                               # loads the file, makes the cached fp4 image
        ibs0, hethet = f_ibs()
        cnt = f_cnt()
        q = L - np.diagonal(hethet).astype(np.int64)
        Q = hethet.astype(np.int64) - L + q[:, None] + q[None, :]
        assert np.array_equal(Q - 2 * ibs0.astype(np.int64), mmt.astype(np.int64)), "sample_ibs and calculateMMt disagree on D"
        assert np.array_equal(cnt[:, 1], np.diagonal(hethet)), "sample_counts and sample_ibs disagree on the heterozygous counts"
        fns = [f_mmt, f_ibs, f_cnt]
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
        rcpp_api.drop_cache()
    out = {"n": n, "L": L, "reps": reps, "device": torch.cuda.get_device_name(0)}
    for name, t in zip(("mmt", "ibs", "sample_counts"), ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    out["ibs_over_mmt"] = out["ibs_ms"] / out["mmt_ms"]

    L2, N = 1000000, n
    p = rng.uniform(0.02, 0.5, L2)
    c = np.stack([rng.multinomial(N, [(1 - x) ** 2, 2 * x * (1 - x), x * x]) for x in p[:4096]], axis=0)
    counts = np.ascontiguousarray(c[rng.integers(0, c.shape[0], L2)], dtype=np.int32)
    rcpp_api.hwe_exact(counts)
    th = []
    for _ in range(reps):
        t0 = time.perf_counter()
        pv = rcpp_api.hwe_exact(counts)
        th.append((time.perf_counter() - t0) * 1e3)
    assert np.all((pv > 0) & (pv <= 1))
    out.update({"hwe_markers": L2, "hwe_individuals": N, "hwe_ms": float(np.median(th)), "hwe_ms_min": float(np.min(th)),
                "hwe_ms_max": float(np.max(th)), "hwe_markers_per_s": L2 / (float(np.median(th)) * 1e-3)})
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
