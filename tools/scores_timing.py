"""Times the exact line-score pass (include/eagle_hip.h section 1b''''i) beside the counting pass on ONE resident synthetic panel, both
files, in one run:

  sample_counts_ms, marker_counts_ms     eagle_sample_counts / eagle_marker_counts: the yardsticks, one read of the same resident images
                                         (M.ascii's and Mt.ascii's), three int32 per line to the host
  sample_scores_T{1,10,64}_ms            eagle_sample_scores with T columns of full-range weights (|w| <= 2^30, four digit planes): the
                                         weights to the device, k_score_digits, k_line_scores_i8, k_scores_finish, n x T int64 back
  marker_scores_T{1,10,64}_ms            eagle_marker_scores likewise on the Mt image, L x T int64 back
  *_over_counts                          each scores time over the counting pass of the same file

From the code the product reads the image once against a digit image of at most 256 rows, so it should cost the image read plus
2 * rows_pad * C * 256 int8 operations.  The eight calls are alternated rep by rep, medians reported; every
scores result is checked against the all-ones identity (n2 - n0 of the counts) on its first column before the clock starts.
Wall-clock times of whole calls, host transfers included.

    python tools/scores_timing.py [n] [L] [reps] [out.json]      (default 10000 262144 10 profiles/r13_scores.json)
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMNS = (1, 10, 64)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "r13_scores.json")
    import torch
    from eagleeverything_amd import rcpp_api
    rng = np.random.default_rng(0)
    W30 = 1 << 30
    with tempfile.TemporaryDirectory() as d:
        fM, fMt = os.path.join(d, "M.ascii"), os.path.join(d, "Mt.ascii")
        G = rng.integers(0, 3, (n, L), dtype=np.uint8)
        nl = np.full((1, 1), ord("\n"), dtype=np.uint8)
        with open(fM, "wb") as f:                                   # n lines of L characters
            for r0 in range(0, n, 256):
                g = G[r0:r0 + 256]
                f.write(np.concatenate([g + ord("0"), np.broadcast_to(nl, (g.shape[0], 1))], axis=1).tobytes())
        with open(fMt, "wb") as f:                                  # L lines of n characters
            for c0 in range(0, L, 4096):
                g = np.ascontiguousarray(G[:, c0:c0 + 4096].T)
                f.write(np.concatenate([g + ord("0"), np.broadcast_to(nl, (g.shape[0], 1))], axis=1).tobytes())
        del G
        dims = (n, L)
        ws = {T: rng.integers(-W30, W30 + 1, (T, L)).astype(np.int32) for T in COLUMNS}
        vs = {T: rng.integers(-W30, W30 + 1, (T, n)).astype(np.int32) for T in COLUMNS}
        names = ["sample_counts", "marker_counts"]
        fns = [lambda: rcpp_api.sample_counts(fM, dims), lambda: rcpp_api.marker_counts(fMt, dims)]
        for T in COLUMNS:
            names += ["sample_scores_T%d" % T, "marker_scores_T%d" % T]
            fns += [lambda T=T: rcpp_api.sample_scores(fM, dims, ws[T]), lambda T=T: rcpp_api.marker_scores(fMt, dims, vs[T])]
        cs, cm = fns[0]().astype(np.int64), fns[1]().astype(np.int64)     # load both files
        assert np.array_equal(rcpp_api.sample_scores(fM, dims, np.ones(L, dtype=np.int32))[:, 0], cs[:, 2] - cs[:, 0])
        assert np.array_equal(rcpp_api.marker_scores(fMt, dims, np.ones(n, dtype=np.int32))[:, 0], cm[:, 2] - cm[:, 0])
        for f in fns[2:]:
            f()                                                     # warm
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
        rcpp_api.drop_cache()
    pad = lambda x: (x + 255) // 256 * 256
    out = {"n": n, "L": L, "reps": reps, "device": torch.cuda.get_device_name(0), "image_bytes": pad(n) * pad(L),
           "int8_mac_per_call": float(pad(n)) * float(L) * 256.0}
    for name, t in zip(names, ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    for T in COLUMNS:
        out["sample_scores_T%d_over_counts" % T] = out["sample_scores_T%d_ms" % T] / out["sample_counts_ms"]
        out["marker_scores_T%d_over_counts" % T] = out["marker_scores_T%d_ms" % T] / out["marker_counts_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
