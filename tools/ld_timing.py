"""Times the LD passes of csrc/eagle_ld.hip beside the k_marker_counts pass, on ONE resident synthetic int8 image in one run:

  counts_ms            eagle_dev_marker_counts: the HBM-bound yardstick (one read of the image)
  band50_ms, band256_ms   eagle_dev_ld_band at window 50 and 256, r2 0.2 (k_ld_tile band mode; (s, q) made once, outside the timing)
  dots20_ms            eagle_dev_ld_dots for k = 20 gathered rows (k_ld_tile picks mode)
  *_over_counts        each against counts_ms; *_TBps: the image's bytes (L x ceil16(n)) over the time, NOT the bytes requested
                       (band mode requests about (128 + pad32(window)) / 128 times the image, most of the excess from L2)

The kernels are alternated rep by rep, medians reported; the results are checked against torch on three blocks of markers first.
These are the device passes the C entry points eagle_ld_window / eagle_ld_dots launch on a resident image; the entry points add the
counting pass, the copy of the result to the host and, for the mask, the host popcount.

    python tools/ld_timing.py [n] [L] [reps]      (default 10000 262144 10)  ->  profiles/r07_ld.json
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    import torch
    from eagleeverything_amd import _lib, rcpp_api
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    vp = C.c_void_p
    for name, args in (("eagle_dev_marker_counts", [vp, vp, C.c_long, C.c_long, C.c_long, vp, vp]),
                       ("eagle_dev_ld_sq", [vp, vp, C.c_long, vp, vp]),
                       ("eagle_dev_ld_band", [vp, vp, C.c_long, C.c_long, C.c_long, vp, C.c_long, C.c_double, vp, C.c_long, vp]),
                       ("eagle_dev_ld_dots", [vp, vp, C.c_long, C.c_long, C.c_long, vp, C.c_long, vp, vp]),
                       ("eagle_dev_gather_rows_i8", [vp, vp, C.c_long, vp, C.c_long, C.c_long, vp, C.c_long, vp])):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = args
    pad = lambda x: (x + 255) // 256 * 256
    dev = torch.device("cuda:0")
    stream = vp(torch.cuda.current_stream().cuda_stream)
    Lp, ld = pad(L), pad(n)
    Mt8 = torch.randint(-1, 2, (Lp, ld), dtype=torch.int8, device=dev)
    Mt8[:, n:] = 0
    Mt8[1::7] = Mt8[0:-1:7].clone()              # every seventh marker a copy of its predecessor: pairs in LD for the check below
    Mt8[L:] = 0
    counts = torch.empty((L, 3), dtype=torch.int32, device=dev)
    sq = torch.empty((L, 2), dtype=torch.int32, device=dev)
    masks = {w: torch.empty((L, (w + 63) // 64), dtype=torch.int64, device=dev) for w in (50, 256)}
    k = 20
    loci = torch.from_numpy(np.random.default_rng(0).integers(0, L, k).astype(np.int32)).to(dev)
    B8 = torch.empty((64, ld), dtype=torch.int8, device=dev)
    dots = torch.empty((L, k), dtype=torch.int32, device=dev)
    img = vp(Mt8.data_ptr())
    f_counts = lambda: lib.eagle_dev_marker_counts(ctx, img, L, n, ld, vp(counts.data_ptr()), stream)
    f_band = {w: (lambda w=w: lib.eagle_dev_ld_band(ctx, img, L, n, ld, vp(sq.data_ptr()), w, 0.2, vp(masks[w].data_ptr()), (w + 63) // 64, stream))
              for w in (50, 256)}
    f_dots = lambda: lib.eagle_dev_ld_dots(ctx, img, L, n, ld, vp(B8.data_ptr()), k, vp(dots.data_ptr()), stream)
    assert f_counts() == 0 and lib.eagle_dev_ld_sq(ctx, vp(counts.data_ptr()), L, vp(sq.data_ptr()), stream) == 0
    assert lib.eagle_dev_gather_rows_i8(ctx, img, ld, vp(loci.data_ptr()), k, 64, vp(B8.data_ptr()), ld, stream) == 0
    assert f_band[50]() == 0 and f_band[256]() == 0 and f_dots() == 0
    torch.cuda.synchronize()

    # the results against torch on three blocks of markers (fp32 products of -1/0/1 summed in fp64 would be slow: int8 -> fp64 matmul)
    for r0 in sorted({0, max(0, L // 2 - 300), max(0, L - 600)}):
        r1 = min(L, r0 + 600)
        G = Mt8[r0:r1, :n].to(torch.float64)
        D = (G @ G.T).to(torch.int64)
        s = sq[r0:r1, 0].to(torch.int64)
        v = n * sq[r0:r1, 1].to(torch.int64) - s * s
        cc = (n * D - s[:, None] * s[None, :]).to(torch.float64)
        ld_pair = (v[:, None] > 0) & (v[None, :] > 0) & (cc * cc > 0.2 * (v.to(torch.float64)[:, None] * v.to(torch.float64)[None, :]))
        for w in (50, 256):
            rows = r1 - r0 - w if r1 < L else r1 - r0       # rows whose whole band lies inside the block (all of them at the end)
            got = masks[w][r0:r0 + rows].cpu().numpy().view(np.uint64)
            bits = np.unpackbits(got.view(np.uint8), axis=1, bitorder="little")[:, :w]
            exp = np.zeros_like(bits)
            lp = ld_pair.cpu().numpy()
            for o in range(1, w + 1):
                m = min(rows, r1 - r0 - o)
                if m > 0:
                    exp[:m, o - 1] = lp[np.arange(m), np.arange(m) + o]
            assert np.array_equal(bits, exp) and exp.any(), "k_ld_tile (band, window %d) differs from torch at marker %d" % (w, r0)
        Gl = Mt8[loci.long(), :n].to(torch.float64)
        assert torch.equal(dots[r0:r1].to(torch.int64), (G @ Gl.T).to(torch.int64)), "k_ld_tile (picks) differs from torch"
        del G, D, Gl

    fns = [f_counts, f_band[50], f_band[256], f_dots]
    for _ in range(2):
        for f in fns:
            assert f() == 0
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts[i].append(e0.elapsed_time(e1))
    image_bytes = L * 16 * ((n + 15) // 16)
    out = {"n": n, "L": L, "reps": reps, "image_bytes": image_bytes, "device": torch.cuda.get_device_name(0)}
    for name, t in zip(("counts", "band50", "band256", "dots20"), ts):
        med = float(np.median(t))
        out.update({name + "_ms": med, name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t)),
                    name + "_TBps": image_bytes / (med * 1e-3) / 1e12})
    for name in ("band50", "band256", "dots20"):
        out[name + "_over_counts"] = out[name + "_ms"] / out["counts_ms"]
    for w in (50, 256):
        out["band%d_int8_ops" % w] = 2.0 * n * L * 128 * 32 * ((w + 31) // 32 + 1) / 128   # 32 x 32 blocks computed, incl. those partly in the band
        out["band%d_POPs" % w] = out["band%d_int8_ops" % w] / (out["band%d_ms" % w] * 1e-3) / 1e15
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r07_ld.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
