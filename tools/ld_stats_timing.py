"""Times eagle_ld_stats (include/eagle_hip.h section 1b'''v) beside eagle_ld_partners on ONE resident synthetic image in one run:

  partners50_ms, partners256_ms      eagle_ld_partners, l = 16, window 50 and 256: the yardstick -- the same r2 band written by k_ld_tile's
                                     r2 mode and read by k_ld_partners, L x 16 int32 and fp64 to the host
  stats50_ms, stats256_ms            eagle_ld_stats without bins: the same band, k_ld_reduce, L uint64 and L int32 to the host
  stats50_bins_ms, stats256_bins_ms  ... with 50 bins of marker offsets (the decay curve): the LDS histogram and its flush as well

The six calls are alternated rep by rep, medians reported.  Before timing, the first markers of the sums are compared with
r_api.ld_stats_host.  Wall-clock times of whole calls on a resident image, host transfers included; no kernel is timed on its own.

    python tools/ld_stats_timing.py [n] [L] [reps] [out.json]       (default 10000 262144 10 profiles/r12_ld_stats.json)
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
    n, L, reps = arg(1, 10000, int), arg(2, 262144, int), arg(3, 10, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r12_ld_stats.json"), str)
    import torch
    from eagleeverything_amd import _lib, r_api, rcpp_api, synth
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    pad = lambda x: (x + 255) // 256 * 256
    dev = torch.device("cuda:0")
    Mt8 = torch.randint(-1, 2, (pad(L), pad(n)), dtype=torch.int8, device=dev)
    Mt8[:, n:] = 0
    Mt8[1::7] = Mt8[0:-1:7].clone()              # every seventh marker a copy of its predecessor: pairs in full LD
    Mt8[L:] = 0
    head = min(L, 600)
    host = Mt8[:head, :n].cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        fMt, dims = os.path.join(d, "Mt.ascii"), (n, L)
        synth.write_sidecar_from_device(lib, ctx, Mt8, L, n, fMt)
        del Mt8
        torch.cuda.empty_cache()
        bins = {w: np.unique(np.rint(np.linspace(1.0, w + 1.0, 51)).astype(np.int64)) for w in (50, 256)}
        fns, names = [], []
        for w in (50, 256):
            fns += [lambda w=w: rcpp_api.ld_partners(fMt, dims, w, 16, 0.0, return_r2=True),
                    lambda w=w: rcpp_api.ld_stats(fMt, dims, w),
                    lambda w=w: rcpp_api.ld_stats(fMt, dims, w, edges=bins[w])]
            names += ["partners%d" % w, "stats%d" % w, "stats%d_bins" % w]
        res = [f() for f in fns]                 # warm-up: the resident image
        for w, (U, cnt, bsum, bpairs) in ((50, res[2]), (256, res[5])):
            rows = head - w if head < L else head                        # markers whose candidates all lie in the block
            hU, hcnt = r_api.ld_stats_host(r_api.ld_band_host(host, w))
            assert np.array_equal(U[:rows], hU[:rows]) and np.array_equal(cnt[:rows], hcnt[:rows]), "eagle_ld_stats differs from numpy"
            assert int(cnt.sum(dtype=np.int64)) == 2 * int(bpairs.sum()), "the bins do not hold every pair once"
            assert int(U.sum(dtype=np.uint64)) == 2 * int(bsum.sum(dtype=np.uint64))
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
    out = {"n": n, "L": L, "reps": reps, "l": 16, "bins": 50, "image_bytes": pad(L) * pad(n),
           "band50_bytes": L * 50 * 8, "band256_bytes": L * 256 * 8, "device": torch.cuda.get_device_name(0),
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the six calls alternated, medians",
           "not_timed": "the kernels on their own, a streamed Mt.ascii, eagle_bed_ld_stats, a map (chrom, pos, max_dist)"}
    for name, t in zip(names, ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    for w in (50, 256):
        out["stats%d_over_partners%d" % (w, w)] = out["stats%d_ms" % w] / out["partners%d_ms" % w]
        out["stats%d_bins_over_partners%d" % (w, w)] = out["stats%d_bins_ms" % w] / out["partners%d_ms" % w]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
