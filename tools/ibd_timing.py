"""Times eagle_ibd (include/eagle_hip.h section 1b'''vii) beside eagle_sample_ibs on ONE resident synthetic M.ascii in one run:

  sample_ibs_ms   eagle_sample_ibs: the yardstick -- the two Gram products over all markers, two n x n int32 matrices to the host
  ibd_totals_ms   eagle_ibd, all pairs, seg_cap = 0: k_ibd_planes_i8 (the image once, two bit planes written), the count pass of
                  k_ibd_walk, the P x 4 pair table to the host, the scan there; no fill pass, no segment table
  ibd_table_ms    eagle_ibd, all pairs, seg_cap = the total: the same, then the offsets to the device, the fill pass and the table to the host
  ibd_list_ms     eagle_ibd with the list of pairs r_api.Relatedness reports (KING phi > 0.0884), seg_cap = that list's total

The panel is a founder mosaic so that segments exist: 8 founder genotype rows with a per-marker allele frequency between 0.1 and 0.5 and
5 % het, every individual a mosaic of founder stretches of 500 to 3,999 markers, 0.1 % of the entries redrawn; 16 chromosomes of equal
length, positions 1,000 base pairs apart; the defaults of r_api.IBD (mode ibs1, min_snp 200, min_kb 1000, max_gap_kb 1000, merge_min_snp
100).  The calls are alternated rep by rep, medians reported.  Before timing, the pairs among the first individuals are compared with
r_api.ibd_host.  Wall-clock times of whole calls on a resident image, host transfers included; no kernel is timed on its own.

    python tools/ibd_timing.py [n] [L] [reps] [out.json]       (default 4096 65536 7 profiles/r15_ibd.json)
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

FOUNDERS, STRETCH, NOISE = 8, (500, 4000), 0.001


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 4096, int), arg(2, 65536, int), arg(3, 7, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r15_ibd.json"), str)
    import torch
    from eagleeverything_amd import _lib, r_api, rcpp_api, synth
    lib = _lib.load()
    ctx = rcpp_api.context(0)
    pad = lambda x: (x + 255) // 256 * 256
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(15)
    freq = torch.rand(L, device=dev, generator=gen) * 0.4 + 0.1

    def draw(rows):
        hom = (torch.rand((rows, L), device=dev, generator=gen) < freq).to(torch.int8) * 2 - 1
        return torch.where(torch.rand((rows, L), device=dev, generator=gen) < 0.05, torch.zeros_like(hom), hom)
    founders = draw(FOUNDERS)
    M8 = torch.zeros((pad(n), pad(L)), dtype=torch.int8, device=dev)
    K = L // STRETCH[0] + 2
    cols = torch.arange(L, device=dev)
    band = 256
    for r0 in range(0, n, band):                 # in bands of individuals: no temporary of image size
        r1 = min(n, r0 + band)
        ends = torch.cumsum(torch.randint(STRETCH[0], STRETCH[1], (r1 - r0, K), device=dev, generator=gen), dim=1)
        ids = torch.randint(0, FOUNDERS, (r1 - r0, K), device=dev, generator=gen)
        k = torch.searchsorted(ends, cols.expand(r1 - r0, L).contiguous(), right=True)
        rows = founders[torch.gather(ids, 1, k), cols]
        redraw = torch.rand((r1 - r0, L), device=dev, generator=gen) < NOISE
        M8[r0:r1, :L] = torch.where(redraw, draw(r1 - r0), rows)
    head = min(n, 8)
    host = M8[:head, :L].cpu().numpy().T.copy()   # (L, head), marker-major as ibd_host takes it
    nchr = 16 if L >= 16 * 1024 else 1
    chrom = (np.arange(L) * nchr // L).astype(np.int32)
    pos = (np.arange(L, dtype=np.int64) - np.searchsorted(chrom, chrom)) * 1000
    p = dict(rcpp_api.IBD_DEFAULTS, min_len=1000000, max_gap=1000000)
    prm = _lib.IbdParams(*[p[f] for f in rcpp_api._IBD_FIELDS])
    with tempfile.TemporaryDirectory() as d:
        fM, dims = os.path.join(d, "M.ascii"), (n, L)
        synth.write_sidecar_from_device(lib, ctx, M8, n, L, fM)
        del M8
        torch.cuda.empty_cache()
        cdims = (C.c_long * 2)(n, L)
        P = n * (n - 1) // 2
        total = C.c_long(0)
        i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

        def ibd(pairs, tab, seg, cap):
            rc = lib.eagle_ibd(ctx, os.fsencode(fM), cdims, pairs.ctypes.data_as(i32) if pairs is not None else None,
                               pairs.shape[0] if pairs is not None else 0, chrom.ctypes.data_as(i32), pos.ctypes.data_as(i64), C.addressof(prm),
                               8.0, tab.ctypes.data_as(i64), seg.ctypes.data_as(i32) if seg is not None else None, cap, C.byref(total))
            if rc:
                raise RuntimeError("eagle_ibd: %d %s" % (rc, lib.eagle_last_error(ctx).decode()))
            return int(total.value)
        geno = {"asciifileM": fM, "dim_of_ascii_M": dims}
        rel = r_api.Relatedness(geno)            # warm-up: the resident image; and the list
        lst = np.ascontiguousarray(rel["pairs"], dtype=np.int32)
        tab = np.zeros((P, 4), dtype=np.int64)
        nseg = ibd(None, tab, None, 0)
        seg = np.zeros((max(nseg, 1), 6), dtype=np.int32)
        ibd(None, tab, seg, nseg)
        hp = r_api.ibd_all_pairs(head)
        htab, hseg = r_api.ibd_host(host, None, hp, chrom, pos, **p)
        ords = hp[:, 0].astype(np.int64) * n - hp[:, 0].astype(np.int64) * (hp[:, 0] + 1) // 2 + (hp[:, 1] - hp[:, 0] - 1)
        assert np.array_equal(tab[ords], htab), "eagle_ibd differs from numpy (pair)"
        assert np.array_equal(seg[:nseg][(seg[:nseg, 0] < head) & (seg[:nseg, 1] < head)], hseg), "eagle_ibd differs from numpy (seg)"
        assert int(tab[:, 0].sum()) == nseg
        fns = [lambda: rcpp_api.sample_ibs(fM, dims), lambda: ibd(None, tab, None, 0), lambda: ibd(None, tab, seg, nseg)]
        names = ["sample_ibs", "ibd_totals", "ibd_table"]
        nlist = nseg_list = 0
        if lst.shape[0]:
            nlist = lst.shape[0]
            ltab = np.zeros((nlist, 4), dtype=np.int64)
            nseg_list = ibd(lst, ltab, None, 0)
            lseg = np.zeros((max(nseg_list, 1), 6), dtype=np.int32)
            fns.append(lambda: ibd(lst, ltab, lseg, nseg_list))
            names.append("ibd_list")
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, f in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[i].append((time.perf_counter() - t0) * 1e3)
    npd = (n + 63) // 64 * 64
    out = {"n": n, "L": L, "reps": reps, "params": p, "blocks": nchr, "pairs": P, "segments": nseg, "list_pairs": nlist, "list_segments": nseg_list,
           "panel": {"founders": FOUNDERS, "stretch_markers": list(STRETCH), "noise": NOISE}, "image_bytes": pad(L) * pad(n),
           "plane_bytes": 2 * ((L + 63) // 64) * npd * 8, "pair_table_bytes": P * 32, "table_bytes": nseg * 24,
           "device": torch.cuda.get_device_name(0),
           "what": "wall-clock times of whole calls on a resident image (host transfers included), the calls alternated, medians",
           "not_timed": "the kernels on their own (see the kernel trace), a streamed M.ascii, eagle_bed_ibd, mode ibs2, other sizes, "
                        "a panel without a map (one block)"}
    for name, t in zip(names, ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    out["ibd_totals_over_sample_ibs"] = out["ibd_totals_ms"] / out["sample_ibs_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
