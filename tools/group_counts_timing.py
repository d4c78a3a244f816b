"""Times the per-group genotype counts (include/eagle_hip.h section 1b''''iii) beside the two passes they sit between, on ONE resident
synthetic Mt.ascii (default n x L = 10,000 x 262,144), in one run:

    marker_counts_ms     eagle_marker_counts: the HBM-bound yardstick (one read of the image, L x 3 int32 to the host)
    ld_dots_ms           eagle_ld_dots for 64 loci: the gather, k_ld_tile<2, true> (the tile k_group_tile is the sibling of), L x 64
                         int32 to the host
    group_counts_K_ms    eagle_group_counts at K = 2, 8, 32, 64 groups: the label upload, k_group_onehot, k_group_tile<1> (K <= 32) or
                         k_group_tile<2>, L x K x 3 int32 to the host

The genotypes are independent draws (allele frequencies 0.2 .. 0.8), the labels uniform over the K groups with a tenth of the
individuals in no group.  The calls are alternated rep by rep, medians reported with min and max.  Before timing, the head of each result
is compared with r_api.group_counts_host.  Wall-clock times of WHOLE calls on a resident image: the result copy of L K 12 bytes (201 MB at
K = 64 and the default size) is part of a call and is not timed apart; no kernel is timed on its own (a kernel trace is a run of its own).

    python tools/group_counts_timing.py [n] [L] [reps] [out.json]      (default 10000 262144 10 profiles/r18_group_counts.json)
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KS = (2, 8, 32, 64)


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 10000, int), arg(2, 262144, int), arg(3, 10, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r18_group_counts.json"), str)
    import torch
    from epistasis_timing import alternate, panel
    from eagleeverything_amd import _lib, r_api, rcpp_api, synth
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    dev = torch.device("cuda:0")
    out = {"reps": reps, "device": torch.cuda.get_device_name(0), "n": n, "L": L,
           "image_bytes": int((L + 255) // 256 * 256) * int((n + 255) // 256 * 256),
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the calls alternated, medians",
           "not_timed": "the kernels on their own, the result copy apart from its call, a streamed Mt.ascii, a VIEW alias, the .bed route, "
                        "eagle_fisher_2x2, other sizes"}
    head = 256
    rng = np.random.default_rng(18)
    labels = {}
    for K in KS:
        lab = rng.integers(0, K, n).astype(np.int32)
        lab[rng.random(n) < 0.1] = -1
        labels[K] = lab
    loci = rng.integers(0, L, 64)
    with tempfile.TemporaryDirectory() as d:
        Mt8 = panel(torch, dev, n, L, 18)
        G = Mt8[:head, :n].cpu().numpy()
        fMt, dims = os.path.join(d, "Mt.ascii"), (n, L)
        synth.write_sidecar_from_device(lib, ctx, Mt8, L, n, fMt)
        del Mt8
        torch.cuda.empty_cache()
        whole = rcpp_api.marker_counts(fMt, dims)            # warm-up: the resident image
        rcpp_api.ld_dots(fMt, dims, loci)
        for K in KS:
            got = rcpp_api.group_counts(fMt, dims, labels[K], K)
            assert np.array_equal(got[:head], r_api.group_counts_host(G, labels[K], K)), "eagle_group_counts differs from numpy at K = %d" % K
            assert np.array_equal(rcpp_api.group_counts(fMt, dims, np.where(labels[K] < 0, 0, labels[K]), K).sum(axis=1), whole), \
                "the groups do not sum to eagle_marker_counts at K = %d" % K
        fns = [lambda: rcpp_api.marker_counts(fMt, dims), lambda: rcpp_api.ld_dots(fMt, dims, loci)]
        fns += [lambda K=K: rcpp_api.group_counts(fMt, dims, labels[K], K) for K in KS]
        names = ["marker_counts", "ld_dots"] + ["group_counts_%d" % K for K in KS]
        for name, t in zip(names, alternate(torch, fns, reps)):
            out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
        for K in KS:
            out["group_counts_%d_result_bytes" % K] = L * K * 12
            out["group_counts_%d_over_marker_counts" % K] = out["group_counts_%d_ms" % K] / out["marker_counts_ms"]
            out["group_counts_%d_over_ld_dots" % K] = out["group_counts_%d_ms" % K] / out["ld_dots_ms"]
        rcpp_api.drop_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
