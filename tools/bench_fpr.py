#!/usr/bin/env python3
"""FPR4AM against the route it replaces, on one MI355X.  Synthetic genotypes of N x LM (default the headline
10,000 x 1,000,000; sparse placeholders + 2-bit sidecars), a trait with 10 planted QTL, q = 1 and q = 3 columns of X, R permutations
(default 200) drawn as FPR4AM draws them.  Per q, in a child process of its own under a time limit:
  (a) AM_traits(Y_perm, X, geno, maxit=2): the only route without FPR4AM -- per-trait EMMA, the batched scan;
  (b) FPR4AM(y, X, geno, numreps=R): wall clock split into MM^T, eigh, Z build, U^T [X | Y], EMMA (of which the grid GEMM), scans, rows.
Both run with algebra="device" (eigh and the n x n products on the GPU), (a) first; ONE run each, no warm-up of either beyond the
context and the resident genotypes (a) leaves.  (b) must return (a)'s decisions: the first pick and extBIC[1] < extBIC[0] of every
permutation.  Prints one JSON document and writes it to profiles/fpr_<N>x<LM>.json.

Usage: tools/bench_fpr.py [N] [LM] [R]      (STEP_TIMEOUT seconds per child, default 500)"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SEED = 101


def child(n, L, R, q):
    import torch
    from eagleeverything_amd import am, emma, host_model, r_api, rcpp_api, synth
    from eagleeverything_amd.sharded import DeviceShard
    sh = DeviceShard(n, L)
    sh.fill_synthetic(seed=2)
    planted = np.linspace(0, L - 1, 12, dtype=np.int64)[1:-1]
    rng = np.random.default_rng(3)
    G = np.stack([sh.Mt8[int(j), :n].cpu().numpy().astype(np.float64) for j in planted], axis=1)
    X = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(q - 1)])
    y = 1.0 + G @ (0.5 * np.where(np.arange(planted.size) % 2 == 0, 1.0, -1.0)) + X[:, 1:].sum(axis=1) + rng.standard_normal(n)
    tmpd = tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
    geno = synth.write_geno_pair_sidecars(tmpd, sh)
    del sh
    torch.cuda.empty_cache()
    host_model.set_algebra("device")
    la = host_model.algebra()
    acc, depth = {}, {"emma": 0}

    def wrap(obj, name, label):
        f = getattr(obj, name)

        def g(*a, **k):
            lab = label
            if name == "mm":
                lab = "  of which the grid GEMM [W | W^2]" if depth["emma"] else "U^T [X | Y]"
            if name == "_emma_eig_batch":
                depth["emma"] += 1
            t = time.perf_counter()
            try:
                return f(*a, **k)
            finally:
                c = acc.setdefault(lab, [0, 0.0])
                c[0] += 1
                c[1] += time.perf_counter() - t
                if name == "_emma_eig_batch":
                    depth["emma"] -= 1
        setattr(obj, name, g)

    for obj, name, label in ((r_api, "calcMMt", "MM^T"), (la, "eigh", "eigh"), (la, "mm", None),
                             (rcpp_api, "spectral_prepare", "Z build"), (emma, "_emma_eig_batch", "EMMA, batched (3 fits per permutation)"),
                             (am, "emma_REMLE_eig", "EMMA REML, per trait"), (am, "emma_MLE_eig", "EMMA ML, per trait"),
                             (rcpp_api, "spectral_scan_traits", "scans"), (rcpp_api, "spectral_rows", "rows")):
        wrap(obj, name, label)

    def phases():
        out = {k: {"calls": c, "seconds": round(s, 4)} for k, (c, s) in sorted(acc.items(), key=lambda kv: -kv[1][1])}
        acc.clear()
        return out

    prng = np.random.default_rng(SEED)
    Y = np.column_stack([y[prng.permutation(n)] for _ in range(R)])
    t = time.perf_counter()
    a = am.AM_traits(Y, X, geno, maxit=2)
    ta = time.perf_counter() - t
    pa = phases()
    rcpp_api._spectral_key.clear()      # (b) builds its own Z: without this it would find (a)'s still resident and skip the build
    t = time.perf_counter()
    b = am.FPR4AM(y, X, geno, numreps=R, seed=SEED)
    tb = time.perf_counter() - t
    pb = phases()
    for f in os.listdir(tmpd):
        os.unlink(os.path.join(tmpd, f))
    os.rmdir(tmpd)
    same_pick = [int(r["all_picks"][0]) == int(j) for r, j in zip(a, b["picks"])]
    same_dec = [(r["extBIC_trace"][1] < r["extBIC_trace"][0]) == bool(g > 1) for r, g in zip(a, b["gamma_star"])]
    print(json.dumps({"q": q, "R": R, "am_traits_s": round(ta, 3), "fpr4am_s": round(tb, 3), "speedup": round(ta / tb, 3),
                      "same_first_pick": int(np.sum(same_pick)), "same_decision": int(np.sum(same_dec)),
                      "setgamma": b["setgamma"], "fpr_at_gamma_1": float(am.fpr_curve(b["gamma_star"], 1.0)[0]),
                      "am_traits_phases": pa, "fpr4am_phases": pb}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(*[int(v) for v in sys.argv[2:6]])
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
    R = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    limit = int(os.environ.get("STEP_TIMEOUT", 500))
    out = {"n": n, "L": L, "R": R, "algebra": "device", "runs": []}
    for q in (1, 3):
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", str(n), str(L), str(R),
                            str(q)], stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print("bench_fpr: the q = %d run ended with status %d; stopping" % (q, p.returncode), file=sys.stderr)
            return p.returncode
        out["runs"].append(json.loads(p.stdout.strip().splitlines()[-1]))
        print("bench_fpr: q = %d: AM_traits %.1f s, FPR4AM %.1f s" % (q, out["runs"][-1]["am_traits_s"], out["runs"][-1]["fpr4am_s"]),
              file=sys.stderr, flush=True)
    dest = os.environ.get("BENCH_FPR_OUT", os.path.join(ROOT, "profiles", "fpr_%dx%d.json" % (n, L)))
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
