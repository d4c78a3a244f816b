"""Times the max(T) permutation pass (include/eagle_hip.h section 1b''''vi) beside the counting pass whose tile it extends, on ONE resident
synthetic Mt.ascii (default n x L = 10,000 x 262,144), in one run:

    group_counts_2_ms    eagle_group_counts at K = 2 (cases / controls): one HBM-bound read of the image
    maxt_cc_ms           eagle_maxt with R = 1,024 seeded permutations of a 0/1 trait: one operand plane, k_maxt_tile<1, 4>
    maxt_qt_ms           eagle_maxt with R = 1,024 of a trait with |t| up to 10^6: three planes, k_maxt_tile<3, 2>

A whole eagle_maxt call is the key and sort kernels, the operand, S and V, the observed pass, the permuted pass, the finish and the copy of
L x 28 + R x 12 bytes to the host.  The genotypes are independent draws (allele frequencies 0.2 .. 0.8).  The calls are alternated rep by
rep, medians reported with min and max.  Before timing, the first markers of each result are compared with r_api.maxt_host (d_obs, V,
key_obs and count1 with ==).  Wall-clock times of WHOLE calls on a resident image; no kernel is timed on its own
(a kernel trace is a run of its own).

    python tools/maxt_timing.py [n] [L] [reps] [out.json]      (default 10000 262144 5 profiles/r23_maxt.json)
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

R = 1024


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 10000, int), arg(2, 262144, int), arg(3, 5, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r23_maxt.json"), str)
    import torch
    from epistasis_timing import alternate, panel
    from eagleeverything_amd import _lib, r_api, rcpp_api, synth
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    dev = torch.device("cuda:0")
    out = {"reps": reps, "device": torch.cuda.get_device_name(0), "n": n, "L": L, "R": R,
           "image_bytes": int((L + 255) // 256 * 256) * int((n + 255) // 256 * 256),
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the calls alternated, medians",
           "not_timed": "any kernel on its own, two planes, strata, the explicit route, a streamed Mt.ascii, a VIEW alias, other sizes"}
    head = 32
    rng = np.random.default_rng(23)
    traits = {"cc": rng.integers(0, 2, n), "qt": rng.integers(-1000000, 1000001, n)}
    lab = traits["cc"].astype(np.int32)
    with tempfile.TemporaryDirectory() as d:
        Mt8 = panel(torch, dev, n, L, 23)
        G = Mt8[:head, :n].cpu().numpy()
        fMt, dims = os.path.join(d, "Mt.ascii"), (n, L)
        synth.write_sidecar_from_device(lib, ctx, Mt8, L, n, fMt)
        del Mt8
        torch.cuda.empty_cache()
        rcpp_api.group_counts(fMt, dims, lab, 2)             # warm-up: the resident image
        for name, t in traits.items():
            got = rcpp_api.maxt(fMt, dims, t, seed=23, R=R)
            want = r_api.maxt_host(G, t, None, None, 23, 1, R)
            for k in ("d_obs", "V", "key_obs", "count1"):
                assert np.array_equal(got[k][:head], want[k]), "eagle_maxt's %s differs from maxt_host (%s)" % (k, name)
            out["maxt_%s_min_count1" % name] = int(got["count1"].min())
        fns = [lambda: rcpp_api.group_counts(fMt, dims, lab, 2)] + [lambda t=t: rcpp_api.maxt(fMt, dims, t, seed=23, R=R) for t in traits.values()]
        names = ["group_counts_2"] + ["maxt_" + k for k in traits]
        for name, t in zip(names, alternate(torch, fns, reps)):
            out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
        for name in names[1:]:
            out[name + "_over_group_counts_2"] = out[name + "_ms"] / out["group_counts_2_ms"]
            out[name + "_tera_int8_mac_per_s"] = float(n) * L * R * (1 if name.endswith("cc") else 3) / (out[name + "_ms"] * 1e9)
        rcpp_api.drop_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
