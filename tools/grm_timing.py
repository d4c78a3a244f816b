"""Times eagle_weighted_gram (include/eagle_hip.h section 1b'''') beside eagle_calculateMMt on ONE resident synthetic M.ascii in one run:

  mmt_ms               eagle_calculateMMt: the yardstick (one fp4 SYRK on the cached operand image, finish, n x n fp64 to the host)
  wgram3_ms            eagle_weighted_gram with standardised weights (r_api.grm_weights of the panel's own counts): three digit planes,
                       each one k_scale_cols_i8 pass over the window and one k_gram_i8ab product on the int8 engine, then
                       k_wgram_finish and n x n int64 to the host (the bytes MM^T sends)
  wgram1_ms            the same with unit weights: one plane
  wgram3_over_mmt, wgram1_over_mmt, wgram3_over_wgram1
                       the ratios; from the code one plane should cost about what k_syrk_i8 costs at this size and three planes
                       about three times that plus the scale passes

The three calls are alternated rep by rep, medians reported; the unit-weight result is checked against the yardstick's matrix and the
three-plane result against the same call on the three planes taken one at a time.  Wall-clock times of whole calls, host transfers
included.

    python tools/grm_timing.py [n] [L] [reps] [out.json]      (default 4096 65536 7 profiles/r09_grm.json)
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
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "r09_grm.json")
    import torch
    from eagleeverything_amd import r_api, rcpp_api
    rng = np.random.default_rng(0)
    counts = np.zeros((L, 3), dtype=np.int64)
    with tempfile.TemporaryDirectory() as d:
        fM = os.path.join(d, "M.ascii")
        block = 256
        p = rng.uniform(0.05, 0.5, L)
        with open(fM, "wb") as f:                                   # n lines of L characters, written in bands of individuals
            for r0 in range(0, n, block):
                g = rng.binomial(2, p[None, :], size=(min(block, n - r0), L)).astype(np.uint8)
                for v in range(3):
                    counts[:, v] += np.sum(g == v, axis=0)
                f.write(np.concatenate([g + ord("0"), np.full((g.shape[0], 1), ord("\n"), dtype=np.uint8)], axis=1).tobytes())
        dims = (n, L)
        q3, scale, used = r_api.grm_weights(counts[:, 0], counts[:, 1], counts[:, 2])
        q1 = np.ones(L, dtype=np.uint32)
        planes = [int(np.any((q3 >> (7 * k)) & 127)) for k in range(3)]
        assert planes == [1, 1, 1], planes
        f_mmt = lambda: rcpp_api.calculateMMt_rcpp(fM, 8.0, 16, np.nan, dims)
        f_w3 = lambda: rcpp_api.weighted_gram(fM, dims, q3)
        f_w1 = lambda: rcpp_api.weighted_gram(fM, dims, q1)
        mmt = f_mmt()                                               # loads the file, makes the cached fp4 image
        Q3, Q1 = f_w3(), f_w1()
        assert np.array_equal(Q1.astype(np.float64), mmt), "weighted_gram with unit weights and calculateMMt disagree"
        parts = sum(rcpp_api.weighted_gram(fM, dims, q3 & np.uint32(127 << (7 * k))) for k in range(3))
        assert np.array_equal(Q3, parts) and np.array_equal(Q3, Q3.T), "the three digit planes do not add up"
        fns = [f_mmt, f_w3, f_w1]
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
        rcpp_api.drop_cache()
    out = {"n": n, "L": L, "reps": reps, "device": torch.cuda.get_device_name(0), "markers_used": int(used.sum()),
           "int8_mac_per_plane": float(n) * float(n + 256) / 2.0 * float(L)}
    for name, t in zip(("mmt", "wgram3", "wgram1"), ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    out["wgram3_over_mmt"] = out["wgram3_ms"] / out["mmt_ms"]
    out["wgram1_over_mmt"] = out["wgram1_ms"] / out["mmt_ms"]
    out["wgram3_over_wgram1"] = out["wgram3_ms"] / out["wgram1_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
