"""Times eagle_tdt (include/eagle_hip.h section 1b''''viii) beside eagle_mendel on ONE resident synthetic M.ascii in one run, on the
pedigree of tools/mendel_timing.py (the same seed and rules: a quarter founders, three generations of children, 0.1 % of the genotypes
redrawn, every 100th recorded father replaced):

  mendel_ms      eagle_mendel over the recorded trios with the per-marker counts, the yardstick: the same planes and the same walk, one
                 marker word kind instead of five (k_ibd_planes_i8, k_mendel_trios<true>, T x 6 and L int32 to the host)
  tdt_ms         eagle_tdt at R = 0: the planes, k_tdt_trios<true> (five ballot groups a word, eight popcounts), k_tdt_finish, T x 6,
                 L x 5 int32 and L fp64 to the host
  tdt_flips_ms   eagle_tdt at R = 1024: the same, then k_tdt_signs, k_tdt_image and k_maxt_tile per band, k_maxt_finish, and count1, maxkey
                 and argmax to the host

The calls are alternated rep by rep, medians reported.  Before timing, the first trios are compared with r_api.tdt_host.  Wall-clock
times of whole calls on a resident image, host transfers included; no kernel is timed on its own (a kernel trace comes from a run of this
script under the profiler with reps = 1).

    python tools/tdt_timing.py [n] [L] [R] [reps] [out.json]       (default 4096 65536 1024 7 profiles/r27_tdt.json)
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

NOISE, WRONG_EVERY = 0.001, 100


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, R, reps = arg(1, 4096, int), arg(2, 65536, int), arg(3, 1024, int), arg(4, 7, int)
    out_path = arg(5, os.path.join(ROOT, "profiles", "r27_tdt.json"), str)
    if n < 16 or n % 8:
        raise SystemExit("n must be a multiple of 8, at least 16")
    import torch
    from eagleeverything_amd import _lib, r_api, rcpp_api, synth
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    pad = lambda x: (x + 255) // 256 * 256
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(16)
    q = n // 4                                           # founders, then three generations of q children
    freq = torch.rand(L, device=dev, generator=gen) * 0.6 + 0.2
    hap = torch.zeros((2, n, L), dtype=torch.int8, device=dev)
    hap[:, :q] = (torch.rand((2, q, L), device=dev, generator=gen) < freq).to(torch.int8)
    trios = np.zeros((3 * q, 3), dtype=np.int32)
    band = 256
    for g in range(1, 4):
        f = torch.randint((g - 1) * q, (g - 1) * q + q // 2, (q,), device=dev, generator=gen)
        m = torch.randint((g - 1) * q + q // 2, g * q, (q,), device=dev, generator=gen)
        for r0 in range(0, q, band):                     # in bands of children: no temporary of image size
            r1 = min(q, r0 + band)
            for h, p in enumerate((f, m)):
                pick = torch.rand((r1 - r0, L), device=dev, generator=gen) < 0.5
                hap[h, g * q + r0:g * q + r1] = torch.where(pick, hap[0, p[r0:r1]], hap[1, p[r0:r1]])
        rows = slice((g - 1) * q, g * q)
        trios[rows, 0] = np.arange(g * q, (g + 1) * q)
        trios[rows, 1], trios[rows, 2] = f.cpu().numpy(), m.cpu().numpy()
    M8 = torch.zeros((pad(n), pad(L)), dtype=torch.int8, device=dev)
    for r0 in range(0, n, band):
        r1 = min(n, r0 + band)
        rows = hap[0, r0:r1] + hap[1, r0:r1] - 1
        redraw = torch.rand((r1 - r0, L), device=dev, generator=gen) < NOISE
        M8[r0:r1, :L] = torch.where(redraw, torch.randint(-1, 2, (r1 - r0, L), dtype=torch.int8, device=dev, generator=gen), rows)
    del hap
    wrong = np.arange(0, trios.shape[0], WRONG_EVERY)
    lo = (trios[wrong, 0] // q - 1) * q                  # the first sire of the child's parental generation
    trios[wrong, 1] = lo + (trios[wrong, 1] - lo + 1) % (q // 2)
    head = np.unique(trios[:4].ravel())
    host = M8[torch.as_tensor(head, device=dev).long(), :L].cpu().numpy().T.copy()      # (L, head), marker-major as the host takes it
    at = {int(i): k for k, i in enumerate(head.tolist())}
    with tempfile.TemporaryDirectory() as d:
        fM = os.path.join(d, "M.ascii")
        synth.write_sidecar_from_device(lib, ctx, M8, n, L, fM)
        del M8
        torch.cuda.empty_cache()
        cdims = (C.c_long * 2)(n, L)
        i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        T = trios.shape[0]
        tab, marker = np.zeros((T, 6), dtype=np.int32), np.zeros(L, dtype=np.int32)
        ttab, tmark, key = np.zeros((T, 6), dtype=np.int32), np.zeros((L, 5), dtype=np.int32), np.zeros(L, dtype=np.float64)
        c1, mk, am = np.zeros(L, dtype=np.int32), np.zeros(max(R, 1), dtype=np.float64), np.zeros(max(R, 1), dtype=np.int32)

        def mendel():
            rc = lib.eagle_mendel(ctx, os.fsencode(fM), cdims, trios.ctypes.data_as(i32), T, 8.0, tab.ctypes.data_as(i32), marker.ctypes.data_as(i32))
            if rc:
                raise RuntimeError("eagle_mendel: %d %s" % (rc, lib.eagle_last_error(ctx).decode()))

        def tdt(flips):
            rc = lib.eagle_tdt(ctx, os.fsencode(fM), cdims, trios.ctypes.data_as(i32), T, None, C.c_uint64(1), 1, flips, 8.0,
                               ttab.ctypes.data_as(i32), tmark.ctypes.data_as(i32), key.ctypes.data_as(f64), c1.ctypes.data_as(i32),
                               mk.ctypes.data_as(f64), am.ctypes.data_as(i32))
            if rc:
                raise RuntimeError("eagle_tdt: %d %s" % (rc, lib.eagle_last_error(ctx).decode()))
        rcpp_api.sample_counts(fM, (n, L))               # warm-up: the resident image
        mendel()
        tdt(0)
        tdt(R)
        local = np.vectorize(at.get)
        want = r_api.tdt_host(host, None, local(trios[:4]))
        assert np.array_equal(ttab[:4], want["trio"]), "eagle_tdt differs from numpy"
        assert int(tmark[:, [0, 2, 4]].sum()) == int(ttab[:, 3].sum()) and int(tmark[:, [1, 3, 4]].sum()) == int(ttab[:, 4].sum())
        assert int(c1.max()) <= R
        fns = [mendel, lambda: tdt(0), lambda: tdt(R)]
        names = ["mendel", "tdt", "tdt_flips"]
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
    npd, ld = (n + 63) // 64 * 64, (T + 15) // 16 * 16
    Tm, Um = tmark[:, [0, 2, 4]].sum(axis=1), tmark[:, [1, 3, 4]].sum(axis=1)
    out = {"n": n, "L": L, "reps": reps, "trios": T, "R": R, "wrong_fathers": int(wrong.size),
           "panel": {"founders": q, "generations": 3, "noise": NOISE, "wrong_father_every": WRONG_EVERY},
           "informative_transmissions_per_marker_median": float(np.median(Tm + Um)), "largest_chisq": float(key.max()),
           "smallest_emp2": float((1 + np.sum(mk[:R] >= key.max())) / (R + 1.0)) if R else None,
           "complete_markers_per_trio_median": float(np.median(ttab[:, 0])),
           "image_bytes": pad(L) * pad(n), "plane_bytes": 2 * ((L + 63) // 64) * npd * 8, "d_image_bytes": ((L + 127) // 128 * 128) * ld,
           "sign_operand_bytes": R * ld, "device": torch.cuda.get_device_name(0),
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the calls alternated, medians",
           "not_timed": "the kernels on their own, a streamed M.ascii, eagle_bed_tdt, a banded image, other sizes"}
    for name, t in zip(names, ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    out["tdt_over_mendel"] = out["tdt_ms"] / out["mendel_ms"]
    out["tdt_flips_over_tdt"] = out["tdt_flips_ms"] / out["tdt_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
