"""Times eagle_roh (include/eagle_hip.h section 1b'''vi) beside eagle_marker_counts on ONE resident synthetic image in one run:

  counts_ms      eagle_marker_counts: the yardstick -- one read of the image by k_marker_counts, L x 3 int32 to the host
  roh_totals_ms  eagle_roh with seg_cap = 0: k_roh_flags (the image once, three bit planes written), the count pass of k_roh_segments,
                 the counts by (individual, block) and ind_out to the host, the scan there; no fill pass, no table
  roh_table_ms   eagle_roh with seg_cap = the total: the same, then the offsets to the device, the fill pass and the table to the host

The image is inbred-like: het rate 5 %, every 100th individual with a planted fully homozygous stretch of 5,000 markers; 16 chromosomes
of equal length, positions 1,000 base pairs apart; default parameters with min_snp lowered to 75.  The three calls are alternated rep by
rep, medians reported.  Before timing, the first individuals of the result are compared with r_api.roh_host.  Wall-clock times of whole
calls on a resident image, host transfers included; no kernel is timed on its own.

    python tools/roh_timing.py [n] [L] [reps] [out.json]       (default 10000 262144 10 profiles/r14_roh.json)
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
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 10000, int), arg(2, 262144, int), arg(3, 10, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r14_roh.json"), str)
    import torch
    from eagleeverything_amd import _lib, r_api, rcpp_api, synth
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    pad = lambda x: (x + 255) // 256 * 256
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(14)
    Mt8 = torch.zeros((pad(L), pad(n)), dtype=torch.int8, device=dev)
    rows = 8192
    for r0 in range(0, L, rows):                 # in row bands: no temporary of image size
        r1 = min(L, r0 + rows)
        hom = torch.rand((r1 - r0, n), device=dev, generator=g) >= 0.05
        sign = torch.randint(0, 2, (r1 - r0, n), device=dev, generator=g, dtype=torch.int8) * 2 - 1
        Mt8[r0:r1, :n] = torch.where(hom, sign, torch.zeros_like(sign))
    span = min(5000, L // 2)
    rng = np.random.default_rng(14)
    for i in range(0, n, 100):
        s = int(rng.integers(0, L - span + 1))
        Mt8[s:s + span, i] = 1
    head = min(n, 8)
    host = Mt8[:L, :head].cpu().numpy()
    nchr = 16 if L >= 16 * 1024 else 1
    chrom = (np.arange(L) * nchr // L).astype(np.int32)
    pos = (np.arange(L, dtype=np.int64) - np.searchsorted(chrom, chrom)) * 1000
    p = dict(rcpp_api.ROH_DEFAULTS, min_snp=75)
    prm = _lib.RohParams(*[p[f] for f in rcpp_api._ROH_FIELDS])
    with tempfile.TemporaryDirectory() as d:
        fMt, dims = os.path.join(d, "Mt.ascii"), (n, L)
        synth.write_sidecar_from_device(lib, ctx, Mt8, L, n, fMt)
        del Mt8
        torch.cuda.empty_cache()
        cdims = (C.c_long * 2)(n, L)
        ind = np.zeros((n, 4), dtype=np.int64)
        total = C.c_long(0)

        def roh(seg, cap):
            rc = lib.eagle_roh(ctx, os.fsencode(fMt), cdims, chrom.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(C.POINTER(C.c_int64)),
                               C.addressof(prm), 8.0, ind.ctypes.data_as(C.POINTER(C.c_int64)),
                               seg.ctypes.data_as(C.POINTER(C.c_int32)) if seg is not None else None, cap, C.byref(total))
            if rc:
                raise RuntimeError("eagle_roh: %d %s" % (rc, lib.eagle_last_error(ctx).decode()))
        rcpp_api.marker_counts(fMt, dims)        # warm-up: the resident image
        roh(None, 0)
        nseg = int(total.value)
        seg = np.zeros((nseg, 6), dtype=np.int32)
        roh(seg, nseg)
        hind, hseg = r_api.roh_host(r_api.roh_classes_mt8(host), chrom, pos, **p)
        assert np.array_equal(ind[:head], hind), "eagle_roh differs from numpy (ind)"
        assert np.array_equal(seg[seg[:, 0] < head], hseg), "eagle_roh differs from numpy (seg)"
        assert int(ind[:, 0].sum()) == nseg
        fns = [lambda: rcpp_api.marker_counts(fMt, dims), lambda: roh(None, 0), lambda: roh(seg, nseg)]
        names = ["counts", "roh_totals", "roh_table"]
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
    nw = (n + 63) // 64
    out = {"n": n, "L": L, "reps": reps, "params": p, "blocks": nchr, "segments": nseg, "image_bytes": pad(L) * pad(n),
           "plane_bytes": 3 * L * nw * 8, "table_bytes": nseg * 24, "counts_by_block_bytes": n * nchr * 4,
           "device": torch.cuda.get_device_name(0),
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the three calls alternated, medians",
           "not_timed": "the kernels on their own, a streamed Mt.ascii, eagle_bed_roh, a panel without a map (one block)"}
    for name, t in zip(names, ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    out["roh_totals_over_counts"] = out["roh_totals_ms"] / out["counts_ms"]
    out["roh_table_over_counts"] = out["roh_table_ms"] / out["counts_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
