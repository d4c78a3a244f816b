#!/usr/bin/env python3
"""Wall-clock medians of every .bed entry point (the ten eagle_bed_* calls and eagle_create_ascii_from_bed) on ONE synthetic fileset,
for the checkout whose root is given: made to compare two builds of the host pipeline (csrc/eagle_ingest.cpp: BedRing, BedRewrite,
BedPanel) process by process.  -> profiles/r16_bed_ring.json holds such a comparison.

    python tools/bed_entry_timing.py gen DIR             writes DIR/panel.bed (4,096 x 65,536, 5 % missing) and DIR/small.bed (2,049 x 20,000)
    python tools/bed_entry_timing.py ROOT DIR OUT.json   times the package under ROOT on them, page cache warm: a warm-up, then 7 rounds of
                                                         all calls in turn; staging windows of 8 MiB, i.e. eight windows per pass

Whole calls, host transfers and file I/O included; no kernel is timed on its own.  Run the two builds alternately, several processes
each: the spread between the processes of ONE build is the yardstick for a difference between the builds."""
import json, os, sys, time
import numpy as np

N, L, REPS = 4096, 65536, 7
RB = (N + 3) // 4
MEM = 4 * (8 << 20) / 1e9          # a quarter of it per window: 8,192 rows, eight windows
NS, LS = 2049, 20000               # the converter's file


def gen(d):
    rng = np.random.default_rng(16)
    for name, n, l in (("panel", N, L), ("small", NS, LS)):
        rb = (n + 3) // 4
        with open(os.path.join(d, name + ".bed"), "wb") as f:
            f.write(b"\x6c\x1b\x01")
            for r0 in range(0, l, 8192):
                nr = min(8192, l - r0)
                codes = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size=(nr, rb * 4), p=[0.45, 0.05, 0.1, 0.4])
                codes[:, n:] = 0
                q = codes.reshape(nr, rb, 4)
                f.write((q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8).tobytes())


def main():
    if sys.argv[1] == "gen":
        return gen(sys.argv[2])
    root, d, out_path = sys.argv[1], sys.argv[2], sys.argv[3]
    sys.path.insert(0, root)
    from eagleeverything_amd import rcpp_api
    import eagleeverything_amd
    assert os.path.dirname(os.path.dirname(os.path.realpath(eagleeverything_amd.__file__))) == os.path.realpath(root), eagleeverything_amd.__file__
    bed, small = os.path.join(d, "panel.bed"), os.path.join(d, "small.bed")
    tag = str(os.getpid())
    rng = np.random.default_rng(3)
    nbr = rng.integers(0, N, size=(N, 16), dtype=np.int32)
    off = rng.integers(1, 200, size=(L, 8)) * rng.choice([-1, 1], size=(L, 8))
    part = np.arange(L)[:, None] + off
    part = np.where((part >= 0) & (part < L), part, -1).astype(np.int32)
    chrom = (np.arange(L) // (L // 4)).astype(np.int32)
    pos = np.arange(L, dtype=np.int64) * 1000
    pairs = np.stack([np.arange(0, 2000, 2), np.arange(1, 2000, 2)], axis=1).astype(np.int32)
    o1, o2 = os.path.join(d, "o1_%s.bed" % tag), os.path.join(d, "o2_%s.bed" % tag)
    fM, fMt = os.path.join(d, "M_%s.ascii" % tag), os.path.join(d, "Mt_%s.ascii" % tag)

    def convert():
        rcpp_api.create_ascii_from_bed(small, fM, fMt, 8.0, [NS, LS])
        rcpp_api.drop_cache()

    calls = {
        "marker_counts": lambda: rcpp_api.bed_marker_counts(bed, (N, L), MEM),
        "sample_counts": lambda: rcpp_api.bed_sample_counts(bed, (N, L), MEM),
        "sample_ibs": lambda: rcpp_api.bed_sample_ibs(bed, (N, L), max_memory_in_Gbytes=MEM),
        "impute_knn": lambda: rcpp_api.bed_impute_knn(bed, (N, L), nbr, 5, 1, o1, max_memory_in_Gbytes=MEM),
        "impute_ldknn": lambda: rcpp_api.bed_impute_ldknn(bed, (N, L), part, 5, 1, 2, o2, max_memory_in_Gbytes=MEM),
        "ld_window": lambda: rcpp_api.bed_ld_window(bed, (N, L), 50, 0.2, None, 1, MEM),
        "ld_partners": lambda: rcpp_api.bed_ld_partners(bed, (N, L), 50, 8, 0.0, None, 1, None, MEM),
        "ld_stats": lambda: rcpp_api.bed_ld_stats(bed, (N, L), 50, None, 1, availmemGb=MEM),
        "roh": lambda: rcpp_api.bed_roh(bed, (N, L), None, chrom, pos, MEM),
        "ibd": lambda: rcpp_api.bed_ibd(bed, (N, L), None, pairs, chrom, pos, MEM),
        "create_ascii_from_bed": convert,
    }
    times = {k: [] for k in calls}
    for k, fn in calls.items():
        fn()                                           # warm-up: the page cache, the kernels' code objects, the staging buffers
    for rep in range(REPS):
        for k, fn in calls.items():
            t = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t) * 1e3)
    for p in (o1, o2, fM, fMt, fM + ".e2b", fMt + ".e2b"):
        if os.path.exists(p):
            os.remove(p)
    out = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in times.items()}
    out["root"] = root
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: round(v["median_ms"], 2) for k, v in out.items() if k != "root"}, sort_keys=True))


if __name__ == "__main__":
    main()
