"""Times eagle_hap_ld (include/eagle_hip.h section 1b''''vii) beside eagle_ld_stats on ONE resident synthetic image in one run:

  stats50_ms, stats256_ms            eagle_ld_stats without bins, window 50 and 256: the yardstick -- the r2 band of k_ld_tile (one int8
                                     product per block pair) and k_ld_reduce, L uint64 and L int32 to the host
  hap50_masks_ms, hap256_masks_ms    eagle_hap_ld, masks only: k_hapld_tile (four int8 products per block pair and the fp64 EM of every
                                     pair), two L x ceil(window / 64) uint64 masks to the host
  hap50_bands_ms, hap256_bands_ms    ... with both fp64 bands as well: two more L x window fp64 arrays written and copied to the host

The six calls are alternated rep by rep, medians reported.  Before timing, the first markers of the masks and bands are compared with
r_api.hap_ld_host, whose iteration counts give em_iterations_mean50 / 256 (the mean EM iterations per defined pair with double
heterozygotes or without, over those markers) and em_iterations_max.  Wall-clock times of whole calls on a resident image, host transfers
included; no kernel is timed on its own.

    python tools/hapld_timing.py [n] [L] [reps] [out.json]       (default 10000 262144 5 profiles/r25_hapld.json)
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
    n, L, reps = arg(1, 10000, int), arg(2, 262144, int), arg(3, 5, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r25_hapld.json"), str)
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
    head = min(L, 300)
    host = Mt8[:head, :n].cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        fMt, dims = os.path.join(d, "Mt.ascii"), (n, L)
        synth.write_sidecar_from_device(lib, ctx, Mt8, L, n, fMt)
        del Mt8
        torch.cuda.empty_cache()
        fns, names = [], []
        for w in (50, 256):
            fns += [lambda w=w: rcpp_api.ld_stats(fMt, dims, w),
                    lambda w=w: rcpp_api.hap_ld(fMt, dims, w),
                    lambda w=w: rcpp_api.hap_ld(fMt, dims, w, bands=True)]
            names += ["stats%d" % w, "hap%d_masks" % w, "hap%d_bands" % w]
        res = [f() for f in fns]                 # warm-up: the resident image
        em = {}
        for w, masks, bands in ((50, res[1], res[2]), (256, res[4], res[5])):
            rows = head - w if head < L else head                        # markers whose partners all lie in the block
            want = r_api.hap_ld_host(host, w)
            for key in ("recomb", "strong", "dprime", "r2"):
                assert np.array_equal(bands[key][:rows], want[key][:rows]), "eagle_hap_ld differs from numpy: " + key
            assert np.array_equal(masks["recomb"], bands["recomb"]) and np.array_equal(masks["counts"], bands["counts"])
            defined = want["dprime"][:rows] > -2.0
            em[w] = (float(want["iterations"][:rows][defined].mean()), int(want["iterations"][:rows].max()), [int(c) for c in bands["counts"]])
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
    out = {"n": n, "L": L, "reps": reps, "image_bytes": pad(L) * pad(n), "band50_bytes": L * 50 * 8, "band256_bytes": L * 256 * 8,
           "device": torch.cuda.get_device_name(0), "tol": 1e-10, "max_iter": 1000, "head_markers": head,
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the six calls alternated, medians",
           "not_timed": "the kernel on its own, a streamed Mt.ascii, HapBlocks' host partition"}
    for w in (50, 256):
        out["em_iterations_mean%d" % w], out["em_iterations_max%d" % w], out["counts%d" % w] = em[w]
    for name, t in zip(names, ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    for w in (50, 256):
        out["hap%d_masks_over_stats%d" % (w, w)] = out["hap%d_masks_ms" % w] / out["stats%d_ms" % w]
        out["hap%d_bands_over_stats%d" % (w, w)] = out["hap%d_bands_ms" % w] / out["stats%d_ms" % w]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
