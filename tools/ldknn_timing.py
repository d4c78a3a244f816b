"""Times LD-kNNi (include/eagle_hip.h section 1b'''iii) beside the calls it is built from, on ONE synthetic fileset in one run:

  ld_window_ms       eagle_ld_window on the ingested Mt.ascii (resident image): the yardstick of the partner table -- the same band of
                     dot products on the int8 MFMA, one bit kept per pair
  ld_partners_ms     eagle_ld_partners on the same file: the band kept as fp64 r2 values (k_ld_tile's r2 mode), k_ld_partners, L x l
                     int32 to the host
  impute_knn_ms      eagle_bed_impute_knn on the .bed file, page cache warm, with the genome-wide table of eagle_knn_rows: the
                     yardstick of the imputation -- the same staging ring and write-behind, k_bed_impute per window
  impute_ldknn_ms    eagle_bed_impute_ldknn on the same file with the partner table: the windows with their halos, k_bed_impute_ldknn

The four calls are alternated rep by rep, medians reported.  Before timing, the first 256 markers of the partner table are compared
with r_api.ld_partners_host and the first 64 markers of the LD-kNNi output with r_api.impute_ldknn_host.  Wall-clock times of whole
calls, host transfers and file I/O included; no kernel is timed on its own.

    python tools/ldknn_timing.py [n] [L] [reps] [out.json] [missing rate] [window] [l] [k]
                                                               (default 4096 65536 7 profiles/r12_ldknn.json 0.05 50 16 5)
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
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 4096, int), arg(2, 65536, int), arg(3, 7, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r12_ldknn.json"), str)
    rate, window, l, k = arg(5, 0.05, float), arg(6, 50, int), arg(7, 16, int), arg(8, 5, int)
    import torch
    from eagleeverything_amd import r_api, rcpp_api
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "panel")
        rb = (n + 3) // 4
        founders = rng.integers(0, 3, size=(16, L)).astype(np.uint8)     # mosaics of 16 founders in segments of 64 markers: markers in LD
        with open(prefix + ".bed", "wb") as f:
            f.write(b"\x6c\x1b\x01")
            lut = np.array([0, 2, 3], dtype=np.uint8)
            for r0 in range(0, L, 4096):
                nr = min(4096, L - r0)
                who = rng.integers(0, 16, size=((nr + 63) // 64, n))
                c = lut[founders[np.repeat(who, 64, axis=0)[:nr], np.arange(r0, r0 + nr)[:, None]]]
                c[rng.random(c.shape) < rate] = 1
                f.write(r_api.pack_bed_codes(c).tobytes())
        bed, dims = prefix + ".bed", (n, L)
        fM, fMt = os.path.join(d, "M.ascii"), os.path.join(d, "Mt.ascii")
        rcpp_api.create_ascii_from_bed(bed, fM, fMt, 8.0, list(dims), True, None)
        ibs0, hethet = rcpp_api.sample_ibs(fM, dims)
        nbr = rcpp_api.knn_rows(ibs0, hethet, 64)
        out_knn, out_ld = os.path.join(d, "knn.bed"), os.path.join(d, "ldknn.bed")
        f_win = lambda: rcpp_api.ld_window(fMt, dims, window, 0.2)
        f_par = lambda: rcpp_api.ld_partners(fMt, dims, window, l, 0.0)
        part = f_par()                                                   # warm-up: resident image, page cache, staging buffers
        f_knn = lambda: rcpp_api.bed_impute_knn(bed, dims, nbr, k, 1, out_knn)
        f_ldk = lambda: rcpp_api.bed_impute_ldknn(bed, dims, part, k, 1, 4, out_ld)
        f_win()
        c_knn, c_ld = f_knn(), f_ldk()
        assert np.array_equal(c_knn.sum(axis=1), c_ld.sum(axis=1)), "the two imputations filled different genotypes"
        Lh = min(L, 256 + window)
        raw = np.fromfile(bed, dtype=np.uint8, count=3 + Lh * rb)[3:].reshape(Lh, rb)
        codes = np.stack([(raw >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(Lh, 4 * rb)[:, :n]
        host_part = r_api.ld_partners_host(np.array([-1, 0, 0, 1], dtype=np.int8)[codes], window, l, 0.0)[0]
        head = min(L, 256)
        assert np.array_equal(part[:head], host_part[:head]), "ld_partners differs from numpy"
        Li = min(L, 64)
        sub = np.where(part[:Li] < Lh, part[:Li], -1)                    # (all of them are: 64 + window <= Lh)
        rows, want = r_api.impute_ldknn_host(codes, np.vstack([sub, np.full((Lh - Li, l), -1, dtype=np.int32)]), k, 1, 4)
        got = np.fromfile(out_ld, dtype=np.uint8, count=3 + Li * rb)
        assert bytes(got[:3]) == b"\x6c\x1b\x01" and np.array_equal(got[3:].reshape(Li, rb), rows[:Li]), "k_bed_impute_ldknn differs from numpy"
        assert np.array_equal(c_ld[:Li], want[:Li])
        fns = [f_win, f_par, f_knn, f_ldk]
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
    out = {"n": n, "L": L, "reps": reps, "missing_rate": rate, "window": window, "l": l, "k": k, "min_overlap": 4, "bed_bytes": 3 + L * rb,
           "n_missing": int(c_ld.sum(dtype=np.int64)), "by_vote": int(c_ld[:, 0].sum(dtype=np.int64)),
           "by_fallback": int(c_ld[:, 1].sum(dtype=np.int64)), "partners_listed": int((part >= 0).sum()),
           "device": torch.cuda.get_device_name(0),
           "what": "wall-clock times of whole calls (file I/O from a warm page cache and host transfers included), the four calls "
                   "alternated, medians; founder-mosaic genotypes in segments of 64 markers",
           "not_timed": "the kernels on their own, a cold-cache file, a streamed Mt.ascii, ImputeBed(local=) as a whole"}
    for name, t in zip(("ld_window", "ld_partners", "impute_knn", "impute_ldknn"), ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    out["ld_partners_over_ld_window"] = out["ld_partners_ms"] / out["ld_window_ms"]
    out["impute_ldknn_over_impute_knn"] = out["impute_ldknn_ms"] / out["impute_knn_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
