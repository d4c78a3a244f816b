"""Times the admixture EM step (include/eagle_hip.h section 1b''''v) beside the counting pass, on ONE resident synthetic Mt.ascii
(default n x L = 4,096 x 65,536), in one run:

    group_counts_2_ms          eagle_group_counts at K = 2: the HBM-bound yardstick, one pass over the image
    admixture_K<K>_s<s>_ms     whole eagle_admixture_em calls at K = 2, 8, 16 with steps = 1 and steps = 11: the staging of Q (n x 16)
                               and F (L x 16) fp64, steps x (k_admix_f, k_admix_q, the two finish kernels), the likelihood-only pass,
                               Q, F and l to the host
    admixture_K<K>_step_ms     (steps = 11 minus steps = 1) / 10: one EM step -- two passes over the image -- by difference

The genotypes are independent draws (allele frequencies 0.2 .. 0.8), the start is r_api.admixture_init.  The calls are alternated rep
by rep, medians reported with min and max.  Before timing, one step on the first 512 markers x all individuals is compared with
r_api.admixture_host within the bounds of tests/admixture_truth.py.  Wall-clock times of WHOLE calls on a resident image; no kernel is
timed on its own (a kernel trace is a run of its own).

    python tools/admixture_timing.py [n] [L] [reps] [out.json]      (default 4096 65536 5 profiles/r21_admixture.json)
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KS = (2, 8, 16)
STEPS = (1, 11)


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 4096, int), arg(2, 65536, int), arg(3, 5, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r21_admixture.json"), str)
    import torch
    from epistasis_timing import alternate, panel
    from eagleeverything_amd import _lib, r_api, rcpp_api, synth
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    dev = torch.device("cuda:0")
    out = {"reps": reps, "device": torch.cuda.get_device_name(0), "n": n, "L": L,
           "image_bytes": int((L + 255) // 256 * 256) * int((n + 255) // 256 * 256),
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the calls alternated, medians",
           "not_timed": "the kernels on their own, a streamed Mt.ascii, a VIEW alias, other sizes, r_api.Admixture's whole loop"}
    head = min(512, L)
    u = 2.0 ** -53
    with tempfile.TemporaryDirectory() as d:
        Mt8 = panel(torch, dev, n, L, 21)
        G = Mt8[:head, :n].cpu().numpy()
        fMt, dims = os.path.join(d, "Mt.ascii"), (n, L)
        synth.write_sidecar_from_device(lib, ctx, Mt8, L, n, fMt)
        fH = os.path.join(d, "head")
        os.makedirs(fH)
        gh = synth.write_geno_pair(fH, G)
        del Mt8
        torch.cuda.empty_cache()
        lab = (np.arange(n) % 2).astype(np.int32)
        rcpp_api.group_counts(fMt, dims, lab, 2)              # warm-up: the resident image
        starts = {}
        for K in KS:
            Q, F = r_api.admixture_init(n, head, K, 21)
            got, want = rcpp_api.admixture_em(gh["asciifileMt"], (n, head), Q, F, 1), r_api.admixture_host(G, Q, F, 1)
            rb = 8.0 * (max(n, head) + K + 16) * u
            assert max(np.max(np.abs(got[i] - want[i]) / want[i]) for i in (0, 1)) <= rb, "eagle_admixture_em differs from admixture_host at K = %d" % K
            assert abs(got[2][1] - want[2][1]) <= 2.0 * n * head * (K + 4) * u + n * head * u * abs(want[2][1])
            starts[K] = r_api.admixture_init(n, L, K, 21)
            rcpp_api.admixture_em(fMt, dims, starts[K][0], starts[K][1], 1)     # warm-up of the call's buffers
        fns = [lambda: rcpp_api.group_counts(fMt, dims, lab, 2)]
        fns += [lambda K=K, s=s: rcpp_api.admixture_em(fMt, dims, starts[K][0], starts[K][1], s) for K in KS for s in STEPS]
        names = ["group_counts_2"] + ["admixture_K%d_s%d" % (K, s) for K in KS for s in STEPS]
        for name, t in zip(names, alternate(torch, fns, reps)):
            out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
        for K in KS:
            step = (out["admixture_K%d_s11_ms" % K] - out["admixture_K%d_s1_ms" % K]) / 10.0
            out["admixture_K%d_step_ms" % K] = step
            out["admixture_K%d_step_over_group_counts_2" % K] = step / out["group_counts_2_ms"]
            out["admixture_K%d_step_ns_per_marker_individual" % K] = step * 1e6 / (L * float(n))
        rcpp_api.drop_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
