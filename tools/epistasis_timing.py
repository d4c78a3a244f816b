"""Times the epistasis scan (include/eagle_hip.h section 1b''''ii) beside the LD passes on the SAME resident synthetic Mt.ascii, in one
run, two configurations:

  pairs   n x L = 4,096 x 16,384 (default)
    ld_window_ms        eagle_ld_window at window 256, r2 0.2: the yardstick -- the band of 256 offsets per marker, one MFMA product per
                        block pair, the mask to the host
    epi_pairs_ms        eagle_epistasis_pairs at the threshold of p = 1e-8, gap 0: k_epi_marker, k_epi_tile<1> over the upper triangle of
                        tile pairs (seven MFMA products per block pair and the 128-bit epilogue for every pair), the per-tile results to the
                        host, k_epi_tile<2> over the tile pairs with hits, the tables to the host
  loci    n x L = 10,000 x 262,144 (default)
    ld_dots_ms          eagle_ld_dots for 64 loci: the gather, k_ld_tile<2, true>, L x 64 int32 to the host
    epi_loci_ms         eagle_epistasis_loci for the same 64 loci with the moments: the gather, k_epi_marker, k_epi_tile<0>, L x 64 fp64 and
                        L x 64 x 5 int64 to the host
    epi_loci_stat_ms    the same with mom_out NULL

The genotypes are independent draws (allele frequencies 0.2 .. 0.8), the trait is standard normal noise plus one planted interaction,
quantised by r_api.quantise_trait.  The calls of a configuration are alternated rep by rep, medians reported.  Before timing, the head of
each result is compared with r_api.epistasis_host.  Wall-clock times of whole calls on a resident image, host transfers included; no
kernel is timed on its own.

    python tools/epistasis_timing.py [n_pairs] [L_pairs] [n_loci] [L_loci] [reps] [out.json]
                                     (default 4096 16384 10000 262144 7 profiles/r17_epistasis.json)
"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def panel(torch, dev, n, L, seed):
    """Marker-major int8 image (pad256(L) x pad256(n)) of independent genotypes, in bands of markers."""
    pad = lambda x: (x + 255) // 256 * 256
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    Mt8 = torch.zeros((pad(L), pad(n)), dtype=torch.int8, device=dev)
    band = 8192
    for r0 in range(0, L, band):
        r1 = min(L, r0 + band)
        f = torch.rand((r1 - r0, 1), device=dev, generator=gen) * 0.6 + 0.2
        a = (torch.rand((r1 - r0, n), device=dev, generator=gen) < f).to(torch.int8)
        b = (torch.rand((r1 - r0, n), device=dev, generator=gen) < f).to(torch.int8)
        Mt8[r0:r1, :n] = a + b - 1
    return Mt8


def trait(torch, Mt8, n, a, b, seed):
    from eagleeverything_amd import r_api
    y = np.random.default_rng(seed).standard_normal(n)
    ga, gb = Mt8[a, :n].cpu().numpy().astype(np.float64), Mt8[b, :n].cpu().numpy().astype(np.float64)
    return r_api.quantise_trait(y + 0.1 * (y.max() - y.min()) * ga * gb)[0]


def alternate(torch, fns, reps):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n1, L1, n2, L2, reps = arg(1, 4096, int), arg(2, 16384, int), arg(3, 10000, int), arg(4, 262144, int), arg(5, 7, int)
    out_path = arg(6, os.path.join(ROOT, "profiles", "r17_epistasis.json"), str)
    import torch
    from scipy import special
    from eagleeverything_amd import _lib, r_api, rcpp_api, synth
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    dev = torch.device("cuda:0")
    out = {"reps": reps, "device": torch.cuda.get_device_name(0),
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the calls of a configuration alternated, medians",
           "not_timed": "the kernels on their own, a streamed Mt.ascii, a VIEW alias, min_stat low enough for many hits, other sizes"}

    def record(prefix, names, ts):
        for name, t in zip(names, ts):
            out.update({prefix + name + "_ms": float(np.median(t)), prefix + name + "_ms_min": float(np.min(t)),
                        prefix + name + "_ms_max": float(np.max(t))})

    # ---- all pairs beside the LD band ----
    head = 192
    with tempfile.TemporaryDirectory() as d:
        Mt8 = panel(torch, dev, n1, L1, 17)
        a, b = 5, 100
        yq = trait(torch, Mt8, n1, a, b, 1)
        G = Mt8[:head, :n1].cpu().numpy().T.copy()
        fMt, dims = os.path.join(d, "Mt.ascii"), (n1, L1)
        synth.write_sidecar_from_device(lib, ctx, Mt8, L1, n1, fMt)
        del Mt8
        torch.cuda.empty_cache()
        min_stat = float(special.fdtri(1.0, n1 - 4.0, 1.0 - 1e-8))
        rcpp_api.marker_counts(fMt, dims)                # warm-up: the resident image
        res = rcpp_api.epistasis_pairs(fMt, dims, yq, min_stat=min_stat)
        rcpp_api.ld_window(fMt, dims, 256, 0.2)
        hres = r_api.epistasis_host(G, yq, min_stat=min_stat)
        sel = (res["hit_ij"] < head).all(axis=1)
        assert np.array_equal(res["hit_ij"][sel], hres["hit_ij"]) and np.array_equal(res["hit_stat"][sel], hres["hit_stat"]), \
            "eagle_epistasis_pairs differs from numpy"
        assert res["max"][:2] == (a, b), "the planted pair is not the maximum"
        ts = alternate(torch, [lambda: rcpp_api.ld_window(fMt, dims, 256, 0.2), lambda: rcpp_api.epistasis_pairs(fMt, dims, yq, min_stat=min_stat)],
                       reps)
        record("pairs_", ["ld_window", "epi_pairs"], ts)
        out["pairs"] = {"n": n1, "L": L1, "pairs": L1 * (L1 - 1) // 2, "ld_band_pairs": int(sum(min(256, L1 - 1 - i) for i in range(L1))),
                        "min_stat": min_stat, "nhits": res["nhits"], "ntested": res["ntested"], "max": list(res["max"]),
                        "image_bytes": int((L1 + 255) // 256 * 256) * int((n1 + 255) // 256 * 256)}
        rcpp_api.drop_cache()

    # ---- 64 loci beside the LD dot products ----
    with tempfile.TemporaryDirectory() as d:
        Mt8 = panel(torch, dev, n2, L2, 18)
        loci = np.random.default_rng(2).integers(0, L2, 64)
        loci[0] = 7
        yq = trait(torch, Mt8, n2, 7, 100, 3)
        rows = np.concatenate((np.arange(head), loci))
        G = Mt8[torch.as_tensor(rows, device=dev).long(), :n2].cpu().numpy().T.copy()
        fMt, dims = os.path.join(d, "Mt.ascii"), (n2, L2)
        synth.write_sidecar_from_device(lib, ctx, Mt8, L2, n2, fMt)
        del Mt8
        torch.cuda.empty_cache()
        rcpp_api.marker_counts(fMt, dims)
        stat, mom = rcpp_api.epistasis_loci(fMt, dims, yq, loci)
        rcpp_api.ld_dots(fMt, dims, loci)
        hres = r_api.epistasis_host(G, yq, loci=np.arange(head, head + 64))
        assert np.array_equal(mom[:head], hres["mom"][:head]), "eagle_epistasis_loci differs from numpy (moments)"
        assert np.array_equal(np.nan_to_num(stat[:head], nan=-1.0), np.nan_to_num(hres["stat"][:head], nan=-1.0)), \
            "eagle_epistasis_loci differs from numpy (stat)"
        assert int(np.nanargmax(stat[:, 0])) == 100, "the planted partner is not the maximum of its locus"
        ts = alternate(torch, [lambda: rcpp_api.ld_dots(fMt, dims, loci), lambda: rcpp_api.epistasis_loci(fMt, dims, yq, loci),
                               lambda: rcpp_api.epistasis_loci(fMt, dims, yq, loci, moments=False)], reps)
        record("loci_", ["ld_dots", "epi_loci", "epi_loci_stat"], ts)
        out["loci"] = {"n": n2, "L": L2, "nloci": 64, "image_bytes": int((L2 + 255) // 256 * 256) * int((n2 + 255) // 256 * 256)}
        rcpp_api.drop_cache()

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
