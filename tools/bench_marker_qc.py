#!/usr/bin/env python3
"""Marker QC kernels (csrc/eagle_qc.hip) at benchmark size, HIP events in one process.  Prints one JSON line:
  counts_ms / gemv_ms / counts_over_gemv   k_marker_counts and eagle_dev_gemv_i8 on the SAME resident n x L image, alternated
                       rep by rep (median of `reps`, min and max beside it).  The counting pass reads what the genotype pass
                       reads and does less arithmetic: the target is counts_ms <= 1.25 x gemv_ms of this very run.
  counts_TBps .......  L * 16 ceil(n/16) bytes read over counts_ms (the padding behind n is not read)
  rows_ms, rows_TBps   k_gather_rows_i8: the Mt image of the kept markers (5 % dropped), bytes read + written over time
  cols_ms, cols_TBps   k_gather_cols_i8: the M image of the kept markers, bytes read + written over time
  bed_call_s, bed_rows_per_s, bed_kernel_ms, bed_kernel_share   eagle_bed_marker_counts on an n x L_bed .bed file (page cache warm):
                       the whole call, and k_bed_marker_counts alone on the same rows already in HBM; the rest of the call is staging
                       (pread into pinned memory, H2D) and the counts coming back
Every result is checked against torch / numpy on a sample before it is timed.
Usage: tools/bench_marker_qc.py [n] [L] [reps] [L_bed]"""
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
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    L_bed = int(sys.argv[4]) if len(sys.argv) > 4 else min(L, 262144)
    import torch
    from eagleeverything_amd import _lib, rcpp_api
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    vp = C.c_void_p
    for name, args in (("eagle_dev_marker_counts", [vp, vp, C.c_long, C.c_long, C.c_long, vp, vp]),
                       ("eagle_dev_bed_marker_counts", [vp, vp, C.c_long, C.c_long, vp, vp]),
                       ("eagle_dev_gather_rows_i8", [vp, vp, C.c_long, vp, C.c_long, C.c_long, vp, C.c_long, vp])):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = args
    pad = lambda x: (x + 255) // 256 * 256
    dev = torch.device("cuda:0")
    stream = vp(torch.cuda.current_stream().cuda_stream)
    out = {"n": n, "L": L, "reps": reps}

    def timed(fns, warm=3):
        """Median / min / max milliseconds of each callable, alternated rep by rep."""
        for _ in range(warm):
            for f in fns:
                assert f() == 0
        ts = [[] for _ in fns]
        for _ in range(reps):
            for k, f in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                ts[k].append(e0.elapsed_time(e1))
        return [(float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in ts]

    # 1. the counting pass against the genotype pass, same image
    Lp, ld = pad(L), pad(n)
    Mt8 = torch.randint(-1, 2, (Lp, ld), dtype=torch.int8, device=dev)
    Mt8[:, n:] = 0
    Mt8[L:] = 0
    counts = torch.full((L, 3), -7, dtype=torch.int32, device=dev)
    v = torch.randn(ld, dtype=torch.float64, device=dev)
    a = torch.empty(Lp, dtype=torch.float64, device=dev)
    f_counts = lambda: lib.eagle_dev_marker_counts(ctx, vp(Mt8.data_ptr()), L, n, ld, vp(counts.data_ptr()), stream)
    f_gemv = lambda: lib.eagle_dev_gemv_i8(ctx, vp(Mt8.data_ptr()), Lp, ld, ld, vp(v.data_ptr()), 1.0, vp(a.data_ptr()), stream)
    assert f_counts() == 0
    torch.cuda.synchronize()
    for r0 in sorted({0, max(0, L // 2 - 2048), max(0, L - 4096)}):
        blk = Mt8[r0:min(L, r0 + 4096), :n]
        exp = torch.stack([(blk == g).sum(dim=1) for g in (-1, 0, 1)], dim=1).to(torch.int32)
        assert torch.equal(counts[r0:r0 + exp.shape[0]], exp), "k_marker_counts differs from torch"
    (c_ms, c_lo, c_hi), (g_ms, g_lo, g_hi) = timed([f_counts, f_gemv])
    read = L * 16 * ((n + 15) // 16)
    out.update(counts_ms=c_ms, counts_ms_min=c_lo, counts_ms_max=c_hi, gemv_ms=g_ms, gemv_ms_min=g_lo, gemv_ms_max=g_hi,
               counts_over_gemv=c_ms / g_ms, counts_target_ratio=1.25, counts_bytes=read, counts_TBps=read / (c_ms * 1e-3) / 1e12,
               gemv_TBps=Lp * ld / (g_ms * 1e-3) / 1e12)
    del counts, v, a

    # 2. compaction at 5 % of the markers dropped
    rng = np.random.default_rng(0)
    keep = np.sort(rng.choice(L, L - int(round(0.05 * L)), replace=False)).astype(np.int32)
    nk = int(keep.size)
    dmap = torch.from_numpy(keep).to(dev)
    sub = torch.empty((pad(nk), ld), dtype=torch.int8, device=dev)
    f_rows = lambda: lib.eagle_dev_gather_rows_i8(ctx, vp(Mt8.data_ptr()), ld, vp(dmap.data_ptr()), nk, pad(nk), vp(sub.data_ptr()), ld, stream)
    assert f_rows() == 0
    torch.cuda.synchronize()
    probe = torch.from_numpy(rng.choice(nk, min(nk, 2000), replace=False).astype(np.int64)).to(dev)
    assert torch.equal(sub[probe], Mt8[dmap.long()[probe]]) and not sub[nk:].any(), "k_gather_rows_i8 differs from the indexing"
    (r_ms, r_lo, r_hi), = timed([f_rows])
    out.update(n_kept=nk, rows_ms=r_ms, rows_ms_min=r_lo, rows_ms_max=r_hi, rows_TBps=(nk * ld + pad(nk) * ld) / (r_ms * 1e-3) / 1e12)
    del sub
    M8 = Mt8.view(-1)[:pad(n) * Lp].view(pad(n), Lp)    # the same bytes as an individual-major image: any values serve the timing
    subM = torch.empty((pad(n), pad(nk)), dtype=torch.int8, device=dev)
    f_cols = lambda: lib.eagle_dev_gather_cols_i8(ctx, vp(M8.data_ptr()), Lp, vp(dmap.data_ptr()), 0, n, nk, vp(subM.data_ptr()), pad(nk), stream)
    assert f_cols() == 0
    torch.cuda.synchronize()
    assert torch.equal(subM[:8, :nk], M8[:8][:, dmap.long()]) and not subM[:8, nk:].any(), "k_gather_cols_i8 differs from the indexing"
    (k_ms, k_lo, k_hi), = timed([f_cols])
    out.update(cols_ms=k_ms, cols_ms_min=k_lo, cols_ms_max=k_hi, cols_TBps=(n * Lp + n * pad(nk)) / (k_ms * 1e-3) / 1e12)
    del subM, M8, Mt8, dmap
    torch.cuda.empty_cache()

    # 3. bed counts: any bytes are valid rows once the unused bit pairs of the last byte are cleared
    rb = (n + 3) // 4
    rows = rng.integers(0, 256, size=(L_bed, rb), dtype=np.uint8)
    if n % 4:
        rows[:, -1] &= (1 << (2 * (n % 4))) - 1
    codes = np.stack([(rows[:2000] >> (2 * q)) & 3 for q in range(4)], axis=2).reshape(-1, 4 * rb)[:, :n]
    exp = np.stack([np.sum(codes == c, axis=1) for c in (0, 2, 3, 1)], axis=1).astype(np.int32)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as d:
        bed = os.path.join(d, "panel.bed")
        with open(bed, "wb") as f:
            f.write(b"\x6c\x1b\x01")
            f.write(rows.tobytes())
        got = rcpp_api.bed_marker_counts(bed, (n, L_bed))      # warm-up: page cache, staging buffers
        assert np.array_equal(got[:2000], exp), "k_bed_marker_counts differs from numpy"
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            rcpp_api.bed_marker_counts(bed, (n, L_bed))
            ts.append(time.perf_counter() - t)
    call_s = float(np.median(ts))
    d_rows = torch.from_numpy(rows).to(dev)
    d_cnt = torch.empty((L_bed, 4), dtype=torch.int32, device=dev)
    f_bed = lambda: lib.eagle_dev_bed_marker_counts(ctx, vp(d_rows.data_ptr()), L_bed, n, vp(d_cnt.data_ptr()), stream)
    assert f_bed() == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_cnt[:2000].cpu().numpy(), exp)
    (b_ms, b_lo, b_hi), = timed([f_bed])
    out.update(L_bed=L_bed, bed_bytes=L_bed * rb, bed_call_s=call_s, bed_call_s_min=float(np.min(ts)), bed_call_s_max=float(np.max(ts)),
               bed_rows_per_s=L_bed / call_s, bed_call_GBps=L_bed * rb / call_s / 1e9, bed_kernel_ms=b_ms, bed_kernel_ms_min=b_lo,
               bed_kernel_ms_max=b_hi, bed_kernel_TBps=L_bed * rb / (b_ms * 1e-3) / 1e12, bed_kernel_share=b_ms * 1e-3 / call_s,
               bed_staging_share=1.0 - b_ms * 1e-3 / call_s)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
