"""Times the saddlepoint pass of the logistic mixed model (include/eagle_hip.h section 1d''') beside the per-marker logistic regression,
on ONE resident synthetic Mt.ascii (default n x L = 4,096 x 65,536), in one run:

    logistic_c<c>_f0_ms          eagle_logistic, maximum likelihood, with c = 1 and 15 covariate columns: the yardstick, a Newton fit
                                 per marker by a wave of the same shape
    glmm_spa_c<c>_cut<k>_ms      eagle_glmm_spa with c = 1 and 15 and cutoff 0 (both tails of every marker solved) and 2 (SAIGE's
                                 screen: a marker with |z| <= 2 ends after the first pass), tol 1e-10, max_iter 50, V = V*: the
                                 staging of X (n x 16 fp64), of mu, 1 - mu, D, resid (n x 4) and A, k_glmm_spa, L x 7 fp64 and
                                 L x 2 int32 to the host

The genotypes are independent draws (allele frequencies 0.2 .. 0.8), the covariates standard normal, the status drawn from a logistic
model on them at a prevalence of about 0.1, mu the covariates-only fit (tau = 0: the n^3 null model is host work and not what this
tool times).  The calls are alternated rep by rep, medians reported with min and max, and with them the mean number of evaluations per
marker and the count of every code.  Before timing, the head of each result is compared with glmm.spa_host (equal codes, r* within
1e-6).  Wall-clock times of WHOLE calls on a resident image; no kernel is timed on its own (a kernel trace is a run of its own).

    python tools/glmm_timing.py [n] [L] [reps] [out.json]      (default 4096 65536 5 profiles/r29_glmm.json)
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CS = (1, 15)
CUTOFFS = (0.0, 2.0)


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 4096, int), arg(2, 65536, int), arg(3, 5, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r29_glmm.json"), str)
    import torch
    from epistasis_timing import alternate, panel
    from eagleeverything_amd import _lib, glmm, r_api, rcpp_api, synth
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    dev = torch.device("cuda:0")
    out = {"reps": reps, "device": torch.cuda.get_device_name(0), "n": n, "L": L, "tol": 1e-10, "max_iter": 50,
           "image_bytes": int((L + 255) // 256 * 256) * int((n + 255) // 256 * 256),
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the calls alternated, medians",
           "not_timed": "the kernel on its own, the null model, the scan for V (vara = NULL here), a streamed Mt.ascii, a VIEW alias, other "
                        "sizes, rare alleles (the panel's alleles are common)"}
    head = 32
    rng = np.random.default_rng(29)
    Xs, sts, mus, As, b0s = {}, {}, {}, {}, {}
    for c in CS:
        X = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])
        coef = np.concatenate([[-2.2], 0.5 / np.sqrt(max(c - 1, 1)) * np.ones(c - 1)])
        st = (rng.random(n) < 1.0 / (1.0 + np.exp(-(X @ coef)))).astype(np.int32)
        b0 = r_api.logistic_null_host(X, st)
        mu = 1.0 / (1.0 + np.exp(-(X @ b0)))
        Xs[c], sts[c], mus[c], b0s[c] = X, st, mu, b0
        As[c] = np.linalg.inv(X.T @ ((mu * (1.0 - mu))[:, None] * X))
    with tempfile.TemporaryDirectory() as d:
        Mt8 = panel(torch, dev, n, L, 29)
        G = Mt8[:head, :n].cpu().numpy()
        fMt, dims = os.path.join(d, "Mt.ascii"), (n, L)
        synth.write_sidecar_from_device(lib, ctx, Mt8, L, n, fMt)
        del Mt8
        torch.cuda.empty_cache()
        rcpp_api.logistic(fMt, dims, sts[1], Xs[1], b0s[1], 0)          # warm-up: the resident image

        def spa(c, cut):
            return glmm.spa(fMt, dims, mus[c], sts[c] - mus[c], Xs[c], As[c], None, cut)

        for c in CS:
            for cut in CUTOFFS:
                stat, info = spa(c, cut)
                hs, hi = glmm.spa_host(G, mus[c], sts[c] - mus[c], Xs[c], As[c], None, cut)
                assert np.array_equal(info[:head, 0], hi[:, 0]), "eagle_glmm_spa's codes differ from spa_host at c = %d" % c
                ok = hi[:, 0] == 0
                assert np.all(np.abs(stat[:head][ok][:, [4, 6]] - hs[ok][:, [4, 6]]) <= 1e-6), "eagle_glmm_spa differs from spa_host at c = %d" % c
                key = "glmm_spa_c%d_cut%d" % (c, int(cut))
                out[key + "_mean_evaluations"] = float(info[:, 1].mean())
                out[key + "_codes"] = {str(int(k)): int(v) for k, v in zip(*np.unique(info[:, 0], return_counts=True))}
            info = rcpp_api.logistic(fMt, dims, sts[c], Xs[c], b0s[c], 0)[1]
            out["logistic_c%d_f0_mean_evaluations" % c] = float(info[:, 1].mean())
        fns = [lambda c=c: rcpp_api.logistic(fMt, dims, sts[c], Xs[c], b0s[c], 0) for c in CS]
        fns += [lambda c=c, cut=cut: spa(c, cut) for c in CS for cut in CUTOFFS]
        names = ["logistic_c%d_f0" % c for c in CS] + ["glmm_spa_c%d_cut%d" % (c, int(cut)) for c in CS for cut in CUTOFFS]
        for name, t in zip(names, alternate(torch, fns, reps)):
            out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
        for name in names:
            ev = out[name + "_mean_evaluations"]
            if ev > 0:
                out[name + "_ns_per_marker_individual_evaluation"] = out[name + "_ms"] * 1e6 / (L * float(n) * ev)
        rcpp_api.drop_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
