"""Times eagle_bed_sample_ibs (include/eagle_hip.h section 1b'''ii) against eagle_sample_ibs (section 1b''') on the same genotypes
in one run: a synthetic SNP-major .bed file with a share of its genotypes missing, and the panel ingested from it.

  bed_ibs_ms           eagle_bed_sample_ibs on the .bed file: the rows through the staging ring, k_bed_pack_fp4 (four operand planes from
                       one read), four fp4 SYRKs, k_bed_ibs_finish, five n x n 32-bit matrices to the host
  bed_ibs_nodist_ms    the same without dist (four matrices to the host), through the C entry
  ibs_ms               eagle_sample_ibs on the resident ingested panel: two SYRKs (the first on the cached operand image), k_f4_abs,
                       k_ibs_finish, two n x n int32 matrices to the host
  bed_over_ibs         bed_ibs_ms / ibs_ms; from the code: twice the Gram work, 2.5 x the bytes to the host, plus the file and the pack
                       passes

The calls are alternated rep by rep, medians reported.  Checked first: the opposite-homozygote counts of the two calls are the same
integers (a missing genotype is no homozygote either way) and ncalled's diagonal is the called genotypes of every individual.
Wall-clock times of whole calls, host transfers and the read of the file (from the page cache) included.

    python tools/bed_ibs_timing.py [n] [L] [reps] [out.json] [missing]     (default 4096 65536 7 profiles/r11_bed_ibs.json 0.05)
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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "r11_bed_ibs.json")
    rate = float(sys.argv[5]) if len(sys.argv) > 5 else 0.05
    import torch
    from eagleeverything_amd import _lib, rcpp_api, synth
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        Mt8 = rng.integers(-1, 2, size=(L, n), dtype=np.int8)
        miss = rng.random((L, n), dtype=np.float32) < rate
        bed = synth.write_bed(os.path.join(d, "panel"), Mt8, missing=miss)
        called = (~miss).sum(axis=0)
        del Mt8, miss
        dims = (n, L)
        fM, fMt = os.path.join(d, "M.ascii"), os.path.join(d, "Mt.ascii")
        n_missing = rcpp_api.create_ascii_from_bed(bed, fM, fMt, 8.0, dims)
        lib, ctx = _lib.load(), rcpp_api.context(0)
        outs = [np.zeros((n, n), dtype=np.int32) for _ in range(4)]
        i32p = C.POINTER(C.c_int32)

        def f_nodist():
            rc = lib.eagle_bed_sample_ibs(ctx, os.fsencode(bed), (C.c_long * 2)(n, L), None, 1, 8.0, *[o.ctypes.data_as(i32p) for o in outs], None)
            assert rc == 0, rc
        f_bed = lambda: rcpp_api.bed_sample_ibs(bed, dims)
        f_ibs = lambda: rcpp_api.sample_ibs(fM, dims)
        ncalled, ibs0, hethet, hetsum, dist = f_bed()
        old0, oldh = f_ibs()
        f_nodist()
        assert np.array_equal(ibs0, old0), "bed_sample_ibs and sample_ibs disagree on the opposite homozygotes"
        assert np.array_equal(np.diagonal(ncalled), called), "ncalled's diagonal is not the called genotypes"
        assert all(np.array_equal(a, b) for a, b in zip(outs, (ncalled, ibs0, hethet, hetsum)))
        assert int(n) * L - int(called.sum()) == n_missing
        fns = [f_bed, f_nodist, f_ibs]
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
        rcpp_api.drop_cache()
    out = {"n": n, "L": L, "reps": reps, "missing_rate": rate, "n_missing": n_missing, "device": torch.cuda.get_device_name(0)}
    for name, t in zip(("bed_ibs", "bed_ibs_nodist", "ibs"), ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    out["bed_over_ibs"] = out["bed_ibs_ms"] / out["ibs_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
