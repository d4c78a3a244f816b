#!/usr/bin/env python3
"""BASELINE configs[4]: the repeated-measures design, AM(Zmat=) with REPS records on each of N individuals x LM SNPs (default
2,000 x 1,000,000 x 5 = 10,000 records; synthetic genotypes as sparse placeholders + 2-bit sidecars, 10 planted QTL as SURVEY 8d).
Phase by phase: MM^T, eigh(D^1/2 K D^1/2), EMMA per iteration (REML, ML), the operand build, the scan -- on the reference-shaped
backend and on the spectral one --, and the selected loci against the planted ones.  Each backend runs in a child process of its
own under a time limit; the first non-zero status ends the script.  Prints one JSON document and writes it to
profiles/r06_c5_repeated[_rREPS].json.

Usage: tools/rm_timing_c5.py [N] [LM] [REPS]      (MAXIT, default 12; STEP_TIMEOUT seconds per backend, default 500)
Run it a second time with REPS = 2: the per-iteration host time must not grow with the records beyond the segment sums."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def child(kind, n, L, reps, maxit):
    import torch
    from eagleeverything_amd import am, host_model, rcpp_api, synth
    from eagleeverything_amd.sharded import DeviceShard
    sh = DeviceShard(n, L)
    sh.fill_synthetic(seed=2)
    planted = np.linspace(0, L - 1, 12, dtype=np.int64)[1:-1]
    rng = np.random.default_rng(3)
    G = np.stack([sh.Mt8[int(j), :n].cpu().numpy().astype(np.float64) for j in planted], axis=1)
    beta = 0.9 * np.where(np.arange(planted.size) % 2 == 0, 1.0, -1.0)
    ind = np.repeat(np.arange(n), reps)
    gen = G @ beta + 0.5 * rng.standard_normal(n)
    y = 1.0 + gen[ind] + 0.8 * rng.standard_normal(ind.size)
    X = np.ones((ind.size, 1))
    tmpd = tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
    geno = synth.write_geno_pair_sidecars(tmpd, sh)
    del sh
    torch.cuda.empty_cache()
    acc = {}

    def wrap(obj, name, label):
        f = getattr(obj, name)

        def g(*a, **k):
            t = time.perf_counter()
            r = f(*a, **k)
            c = acc.setdefault(label, [0, 0.0])
            c[0] += 1
            c[1] += time.perf_counter() - t
            return r
        setattr(obj, name, g)

    for obj, name, label in ((rcpp_api, "calculateMMt_rcpp", "MM^T (cold: sidecar -> HBM -> MM^T -> host)"),
                             (host_model.ZModel, "__init__", "eigh(D^1/2 K D^1/2), once per run"),
                             (host_model, "segment_sums", "segment sums Z^T [X | y] (the n_obs-sized work)"),
                             (am, "calcVC", "EMMA REML per iteration (grid + roots)"),
                             (am, "calc_extBIC", "EMMA ML + extBIC per iteration"),
                             (host_model, "scan_operands_z", "operand build S, V, a_hat (t x t)"),
                             (host_model, "calculateMMt_sqrt_and_sqrtinv", "  of which K^(1/2), K^(-1/2) (memoised after the first)"),
                             (rcpp_api, "calculate_a_and_vara_rcpp", "scan: eagle_calculate_a_and_vara (PCIe included)"),
                             (rcpp_api, "spectral_prepare", "spectral: Z~ = Mt (D^1/2 U~ / sqrt d_max), once per run"),
                             (rcpp_api, "spectral_scan_weights", "spectral: the scan (one pass over Z~)"),
                             (rcpp_api, "extract_geno_rcpp", "extract_geno")):
        wrap(obj, name, label)
    backend = am.SpectralBackend() if kind == "spectral" else am.HipBackend()
    t = time.perf_counter()
    r = am.AM(y, X, geno, maxit=maxit, backend=backend, Zmat=ind)
    tot = time.perf_counter() - t
    for f in os.listdir(tmpd):
        os.unlink(os.path.join(tmpd, f))
    os.rmdir(tmpd)
    want = sorted(int(p) + 1 for p in planted)
    print(json.dumps({"total_s": round(tot, 3), "iterations": len(r["extBIC_trace"]), "selected_loci": r["selected_loci"], "planted": want,
                      "planted_found": sorted(set(want) & set(r["selected_loci"])),
                      "phases": {k: {"calls": c, "seconds": round(s, 4)} for k, (c, s) in sorted(acc.items(), key=lambda kv: -kv[1][1])}}))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], *[int(v) for v in sys.argv[3:7]])
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    maxit = int(os.environ.get("MAXIT", 12))
    limit = int(os.environ.get("STEP_TIMEOUT", 500))
    out = {"n_individuals": n, "L": L, "records_per_individual": reps, "n_obs": n * reps, "runs": {}}
    for kind in ("hip", "spectral"):
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", kind, str(n), str(L),
                            str(reps), str(maxit)], stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print("rm_timing_c5: the %s run ended with status %d; stopping" % (kind, p.returncode), file=sys.stderr)
            return p.returncode
        out["runs"][kind] = json.loads(p.stdout.strip().splitlines()[-1])
        print("rm_timing_c5: %s done in %.1f s" % (kind, out["runs"][kind]["total_s"]), file=sys.stderr, flush=True)
    out["same_loci_on_both_backends"] = out["runs"]["hip"]["selected_loci"] == out["runs"]["spectral"]["selected_loci"]
    name = "r06_c5_repeated.json" if reps == 5 else "r06_c5_repeated_r%d.json" % reps
    dest = os.environ.get("RM_TIMING_OUT", os.path.join(ROOT, "profiles", name))
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
