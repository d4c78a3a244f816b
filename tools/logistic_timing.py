"""Times the per-marker logistic regression (include/eagle_hip.h section 1b''''iv) beside the counting pass it extends, on ONE resident
synthetic Mt.ascii (default n x L = 4,096 x 65,536), in one run:

    group_counts_2_ms        eagle_group_counts at K = 2 (cases / controls): what CaseControl costs, the HBM-bound yardstick
    logistic_c<c>_f<f>_ms    eagle_logistic with c = 1, 4, 15 covariate columns (the intercept among them) and firth = 0 (ML) and 2
                             (fallback), tol 1e-10, max_iter 50: the staging of X (n x 16 fp64) and status, k_logit_irls<f>, L x 4 fp64
                             and L x 2 int32 to the host

The genotypes are independent draws (allele frequencies 0.2 .. 0.8), the covariates standard normal, the status drawn from a logistic
model on them with a tenth of the individuals not used.  The calls are alternated rep by rep, medians reported with min and max, and
with them the mean number of evaluations per marker and how many markers took the Firth fit.  Before timing, the head of each result
is compared with r_api.logistic_host (|gamma| within 1e-8, equal codes).  Wall-clock times of WHOLE calls on a resident image; no
kernel is timed on its own (a kernel trace is a run of its own).

    python tools/logistic_timing.py [n] [L] [reps] [out.json]      (default 4096 65536 5 profiles/r19_logistic.json)
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CS = (1, 4, 15)
FIRTH = (0, 2)


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 4096, int), arg(2, 65536, int), arg(3, 5, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r19_logistic.json"), str)
    import torch
    from epistasis_timing import alternate, panel
    from eagleeverything_amd import _lib, r_api, rcpp_api, synth
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    dev = torch.device("cuda:0")
    out = {"reps": reps, "device": torch.cuda.get_device_name(0), "n": n, "L": L, "tol": 1e-10, "max_iter": 50,
           "image_bytes": int((L + 255) // 256 * 256) * int((n + 255) // 256 * 256),
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the calls alternated, medians",
           "not_timed": "the kernel on its own, firth = 1, a streamed Mt.ascii, a VIEW alias, other sizes, a panel with many separated markers"}
    head = 64
    rng = np.random.default_rng(19)
    Xs, sts, b0s = {}, {}, {}
    for c in CS:
        X = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])
        coef = np.concatenate([[-0.2], 0.8 / np.sqrt(max(c - 1, 1)) * np.ones(c - 1)])
        st = (rng.random(n) < 1.0 / (1.0 + np.exp(-(X @ coef)))).astype(np.int32)
        st[rng.random(n) < 0.1] = -1
        Xs[c], sts[c] = X, st
        b0s[c] = r_api.logistic_null_host(X[st >= 0], st[st >= 0])
    with tempfile.TemporaryDirectory() as d:
        Mt8 = panel(torch, dev, n, L, 19)
        G = Mt8[:head, :n].cpu().numpy()
        fMt, dims = os.path.join(d, "Mt.ascii"), (n, L)
        synth.write_sidecar_from_device(lib, ctx, Mt8, L, n, fMt)
        del Mt8
        torch.cuda.empty_cache()
        rcpp_api.group_counts(fMt, dims, sts[1], 2)          # warm-up: the resident image
        for c in CS:
            for f in FIRTH:
                stat, info = rcpp_api.logistic(fMt, dims, sts[c], Xs[c], b0s[c], f)
                hs, hi = r_api.logistic_host(G, sts[c], Xs[c], f, beta0=b0s[c])
                ok = hi[:, 0] % 256 == 0
                assert np.array_equal(info[:head, 0], hi[:, 0]), "eagle_logistic's codes differ from logistic_host at c = %d" % c
                assert np.all(np.abs(stat[:head][ok, 0] - hs[ok, 0]) <= 1e-8), "eagle_logistic differs from logistic_host at c = %d" % c
                key = "logistic_c%d_f%d" % (c, f)
                out[key + "_mean_evaluations"] = float(info[:, 1].mean())
                out[key + "_firth_markers"] = int((info[:, 0] >= 256).sum())
                out[key + "_not_converged"] = int((info[:, 0] % 256 != 0).sum())
        fns = [lambda: rcpp_api.group_counts(fMt, dims, sts[1], 2)]
        fns += [lambda c=c, f=f: rcpp_api.logistic(fMt, dims, sts[c], Xs[c], b0s[c], f) for c in CS for f in FIRTH]
        names = ["group_counts_2"] + ["logistic_c%d_f%d" % (c, f) for c in CS for f in FIRTH]
        for name, t in zip(names, alternate(torch, fns, reps)):
            out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
        for name in names[1:]:
            out[name + "_over_group_counts_2"] = out[name + "_ms"] / out["group_counts_2_ms"]
            out[name + "_ns_per_marker_individual_evaluation"] = out[name + "_ms"] * 1e6 / (L * float(n) * out[name + "_mean_evaluations"])
        rcpp_api.drop_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
