"""Times pairwise-complete LD from a .bed file beside the panel's LD on the SAME genotypes, entry point against entry point, in one run:

  ld50_ms, ld256_ms            rcpp_api.ld_window on the ingested panel (Mt.ascii resident after the warm-up), window 50 and 256, r2 0.2
  bed_ld50_ms, bed_ld256_ms    rcpp_api.bed_ld_window on the .bed file the panel was ingested from (page cache warm), min_overlap n // 10:
                               the file's trip through pinned memory, k_bed_ld_pack, k_bedld_tile (six products per pair, the block
                               offsets two at a time), the mask's copy to the host and its popcount
  *_over_ld                    each bed_ld time against the ld time of the same window

Both are host wall-clock times of the whole call (both calls synchronise before they return), alternated rep by rep, medians
reported.  Before timing, the two masks are compared where they must agree: on the markers without a missing call the pair's own
counts are the panel's, so a pair of two such markers has the same bit.

    python tools/bed_ld_timing.py [n] [L] [reps] [missing]      (default 10000 262144 7 0.05)  ->  profiles/r12_bed_ld.json
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
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    rate = float(sys.argv[4]) if len(sys.argv) > 4 else 0.05
    import torch
    from eagleeverything_amd import r_api, rcpp_api, synth
    rng = np.random.default_rng(12)
    with tempfile.TemporaryDirectory() as tmp:
        Mt8 = synth.genotypes_marker_major(n, L, seed=12)
        Mt8[1::7] = Mt8[0:-1:7]                       # every seventh marker a copy of its predecessor: pairs in LD
        clean = np.arange(L) % 5 == 0                 # a fifth of the markers without a missing call, for the check below
        miss = np.zeros((L, n), dtype=bool)
        for r0 in range(0, L, 8192):
            miss[r0:r0 + 8192] = rng.random((min(8192, L - r0), n)) < rate
        miss[clean] = False
        bed = synth.write_bed(os.path.join(tmp, "panel"), Mt8, missing=miss)
        del Mt8, miss
        geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=tmp)
        dims = (n, L)
        mo = max(2, n // 10)
        fns, names = [], []
        for w in (50, 256):
            fns.append(lambda w=w: rcpp_api.ld_window(geno["asciifileMt"], dims, w, 0.2))
            fns.append(lambda w=w: rcpp_api.bed_ld_window(bed, dims, w, 0.2, None, mo))
            names += ["ld%d" % w, "bed_ld%d" % w]
        for w, (f_ld, f_bed) in zip((50, 256), ((fns[0], fns[1]), (fns[2], fns[3]))):
            a, b = f_ld(), f_bed()                    # the warm-up, and the check
            for o in range(1, w + 1):
                both = clean[:L - o] & clean[o:]
                bit_a = (a[:L - o, (o - 1) // 64] >> np.uint64((o - 1) % 64)) & np.uint64(1)
                bit_b = (b[:L - o, (o - 1) // 64] >> np.uint64((o - 1) % 64)) & np.uint64(1)
                assert np.array_equal(bit_a[both], bit_b[both]), "bed_ld_window differs from ld_window at offset %d" % o
            assert a.any() and b.any()
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append(1e3 * (time.perf_counter() - t0))
        out = {"n": n, "L": L, "reps": reps, "missing": rate, "min_overlap": mo, "bed_bytes": 3 + L * ((n + 3) // 4),
               "device": torch.cuda.get_device_name(0)}
        for name, t in zip(names, ts):
            out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
        for w in (50, 256):
            out["bed_ld%d_over_ld" % w] = out["bed_ld%d_ms" % w] / out["ld%d_ms" % w]
        rcpp_api.drop_cache()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r12_bed_ld.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
