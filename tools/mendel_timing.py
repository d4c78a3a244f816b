"""Times eagle_mendel and eagle_parentage (include/eagle_hip.h section 1b'''viii) beside eagle_sample_counts on ONE resident synthetic
M.ascii in one run:

  sample_counts_ms   eagle_sample_counts: the yardstick -- one pass over the image, an n x 3 int32 table to the host
  mendel_ms          eagle_mendel over the recorded trios with the per-marker counts: k_ibd_planes_i8 (the image once, two bit planes
                     written), k_mendel_trios<true>, the T x 6 table and the L marker counts to the host
  mendel_trios_ms    the same without the per-marker counts (marker_out NULL: k_mendel_trios<false>)
  parentage_ms       eagle_parentage, n_o offspring against n_s sires x n_d dams: the planes, three k_plane_gather, k_parentage,
                     k_parentage_finish, the n_o x 8 rows to the host

The panel is a simulated pedigree: a quarter of the individuals are founders (allele frequencies 0.2 .. 0.8), the rest three
generations of children, each drawing one allele per marker from a sire of the first half and a dam of the second half of the
generation before; 0.1 % of the genotypes are redrawn afterwards (genotyping errors), and every 100th recorded father is replaced by
another sire.  The offspring are the first n_o individuals of the last generation, the candidates the halves of the generation before.
The calls are alternated rep by rep, medians reported.  Before timing, the first trios and a small assignment are compared with
r_api.mendel_host / r_api.parentage_host.  Wall-clock times of whole calls on a resident image, host transfers included; no kernel is
timed on its own.

    python tools/mendel_timing.py [n] [L] [n_o] [reps] [out.json]       (default 4096 65536 256 7 profiles/r16_mendel.json)
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
    n, L, n_o, reps = arg(1, 4096, int), arg(2, 65536, int), arg(3, 256, int), arg(4, 7, int)
    out_path = arg(5, os.path.join(ROOT, "profiles", "r16_mendel.json"), str)
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
    true_fathers = trios[:, 1].copy()
    wrong = np.arange(0, trios.shape[0], WRONG_EVERY)
    lo = (trios[wrong, 0] // q - 1) * q                  # the first sire of the child's parental generation
    trios[wrong, 1] = lo + (trios[wrong, 1] - lo + 1) % (q // 2)
    n_o = min(n_o, q)
    offspring = np.arange(3 * q, 3 * q + n_o, dtype=np.int32)
    sires = np.arange(2 * q, 2 * q + q // 2, dtype=np.int32)
    dams = np.arange(2 * q + q // 2, 3 * q, dtype=np.int32)
    head = np.unique(np.concatenate((trios[:4].ravel(), offspring[:2], sires[:64], dams[:64])))
    host = M8[torch.as_tensor(head, device=dev).long(), :L].cpu().numpy().T.copy()      # (L, head), marker-major as the host takes it
    at = {int(i): k for k, i in enumerate(head.tolist())}
    with tempfile.TemporaryDirectory() as d:
        fM, dims = os.path.join(d, "M.ascii"), (n, L)
        synth.write_sidecar_from_device(lib, ctx, M8, n, L, fM)
        del M8
        torch.cuda.empty_cache()
        cdims = (C.c_long * 2)(n, L)
        i32 = C.POINTER(C.c_int32)
        T = trios.shape[0]
        tab, marker, best = np.zeros((T, 6), dtype=np.int32), np.zeros(L, dtype=np.int32), np.zeros((n_o, 2, 4), dtype=np.int32)

        def mendel(with_markers):
            rc = lib.eagle_mendel(ctx, os.fsencode(fM), cdims, trios.ctypes.data_as(i32), T, 8.0, tab.ctypes.data_as(i32),
                                  marker.ctypes.data_as(i32) if with_markers else None)
            if rc:
                raise RuntimeError("eagle_mendel: %d %s" % (rc, lib.eagle_last_error(ctx).decode()))

        def parentage():
            rc = lib.eagle_parentage(ctx, os.fsencode(fM), cdims, offspring.ctypes.data_as(i32), n_o, sires.ctypes.data_as(i32), sires.size,
                                     dams.ctypes.data_as(i32), dams.size, 1, 0, 8.0, best.ctypes.data_as(i32))
            if rc:
                raise RuntimeError("eagle_parentage: %d %s" % (rc, lib.eagle_last_error(ctx).decode()))
        rcpp_api.sample_counts(fM, dims)                 # warm-up: the resident image
        mendel(True)
        parentage()
        local = np.vectorize(at.get)
        htab, _ = r_api.mendel_host(host, None, local(trios[:4]))
        assert np.array_equal(tab[:4], htab), "eagle_mendel differs from numpy"
        assert int(marker.sum()) == int(tab[:, 5].sum())
        small = rcpp_api.parentage(fM, dims, offspring[:2], sires[:64], dams[:64])
        hsmall = r_api.parentage_host(host, None, local(offspring[:2]), local(sires[:64]), local(dams[:64]))
        hsmall[:, :, :2] = np.where(hsmall[:, :, :2] >= 0, head[np.maximum(hsmall[:, :, :2], 0)], -1)
        assert np.array_equal(small, hsmall), "eagle_parentage differs from numpy"
        truth = {int(c): (int(f), int(m)) for (c, _, m), f in zip(trios.tolist(), true_fathers.tolist())}
        found = sum(1 for c, row in zip(offspring.tolist(), best[:, 0].tolist()) if (row[0], row[1]) == truth[c])
        fns = [lambda: rcpp_api.sample_counts(fM, dims), lambda: mendel(True), lambda: mendel(False), parentage]
        names = ["sample_counts", "mendel", "mendel_trios", "parentage"]
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
    npd = (n + 63) // 64 * 64
    bad = np.zeros(T, dtype=bool)
    bad[wrong] = True
    out = {"n": n, "L": L, "reps": reps, "trios": T, "wrong_fathers": int(wrong.size), "offspring": int(n_o), "sires": int(sires.size),
           "dams": int(dams.size), "candidates_per_offspring": int(sires.size) * int(dams.size), "true_parents_found": found,
           "panel": {"founders": q, "generations": 3, "noise": NOISE, "wrong_father_every": WRONG_EVERY},
           "median_errors_recorded_right": float(np.median(tab[~bad, 5])), "median_errors_recorded_wrong": float(np.median(tab[bad, 5])),
           "median_best_errors": float(np.median(best[:, 0, 2])), "median_runner_up_errors": float(np.median(best[:, 1, 2])),
           "image_bytes": pad(L) * pad(n), "plane_bytes": 2 * ((L + 63) // 64) * npd * 8, "device": torch.cuda.get_device_name(0),
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the calls alternated, medians",
           "not_timed": "the kernels on their own, a streamed M.ascii, eagle_bed_mendel, eagle_bed_parentage, single-parent assignment, other sizes"}
    for name, t in zip(names, ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
