#!/usr/bin/env python3
"""ReadMarker(type="PLINKbed") against ReadMarker(type="text") on the same genotypes, on one MI355X -> profiles/bed_ingest.json.

    python tools/bench_bed.py [--shapes 5000x200000,10000x200000] [--big 10000x1000000] [--dir DIR] [--out FILE]

Per shape: the panel is written both ways by synth (a "0 1 2" table, 2 bytes per genotype, and a .bed fileset, 2 bits), a small
panel goes through both routes first (warm-up: context, staging buffers, code objects), then bed, text, bed, text.  Recorded: wall
time and input bytes of every run, whether all four outputs (both text files, both sidecar payloads) are identical between the
routes, and the first calculateMMt_rcpp after a bed ingestion (served by the adopted image) next to the same call after
drop_cache (served by the sidecar).  Then k_bed_decode alone: one more bed ingestion of the first shape in a child process under
`rocprofv3 --kernel-trace --stats`, the kernel's bytes read plus written computed here from the shapes, over its total time, next
to the 8 TB/s HBM figure -- the kernel's share of the memory roof, not a claim about the call.  --big: one bed ingestion at that
shape (wall time only), or the reason it was not run.  A shape whose files do not fit the free space of --dir is skipped, and says so.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def pad(x, m=256):
    return (x + m - 1) // m * m


def write_table(path, Mt8, block=4096):
    """individuals x markers, '0' / '1' / '2' separated by one blank."""
    L, n = Mt8.shape
    with open(path, "wb") as f:
        for r0 in range(0, n, block):
            g = np.ascontiguousarray(Mt8[:, r0:r0 + block].T) + 1 + ord("0")
            buf = np.full((g.shape[0], 2 * L), ord(" "), dtype=np.uint8)
            buf[:, 0::2] = g
            buf[:, -1] = ord("\n")
            f.write(buf.tobytes())


def same_outputs(a, b):
    out = {}
    for name in ("M.ascii", "Mt.ascii"):
        out[name] = _same(os.path.join(a, name), os.path.join(b, name), 0)
        out[name + ".e2b payload"] = _same(os.path.join(a, name + ".e2b"), os.path.join(b, name + ".e2b"), 64)
    return out


def _same(fa, fb, skip, chunk=1 << 26):
    if not (os.path.exists(fa) and os.path.exists(fb)) or os.path.getsize(fa) != os.path.getsize(fb):
        return False
    with open(fa, "rb") as a, open(fb, "rb") as b:
        a.seek(skip), b.seek(skip)
        while True:
            x, y = a.read(chunk), b.read(chunk)
            if x != y:
                return False
            if not x:
                return True


def kernel_bytes(n, L):
    """k_bed_decode over one ingestion with both images resident: the bed rows in, the padded int8 image of Mt and the sidecar rows out."""
    rb, rb16 = (n + 3) // 4, pad((n + 3) // 4, 16)
    return {"read": L * rb, "written": pad(L) * pad(n) + L * rb16}


def child_ingest(bed, outdir):
    from eagleeverything_amd import r_api, rcpp_api
    t0 = time.perf_counter()
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=outdir)
    wall = time.perf_counter() - t0
    assert geno is not None
    rcpp_api.close_all()
    print(json.dumps({"wall_s": wall}))


def kernel_stats(bed, work, n, L):
    prof = os.path.join(work, "prof")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "bed", "--",
           sys.executable, os.path.abspath(__file__), "--child-ingest", bed, "--dir", os.path.join(work, "prof_out")]
    os.makedirs(os.path.join(work, "prof_out"), exist_ok=True)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        return {"error": "rocprofv3 run failed (%d): %s" % (r.returncode, (r.stderr or r.stdout)[-400:])}
    files = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"error": "no kernel_stats.csv written"}
    out = {"kernels": {}}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            for k in ("k_bed_decode", "k_transpose_i8", "k_encode_ascii", "k_pack2b"):
                if k + "(" in row["Name"] or row["Name"].startswith(k):
                    out["kernels"][k] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6}
    dec = out["kernels"].get("k_bed_decode")
    if dec:
        b = kernel_bytes(n, L)
        rate = (b["read"] + b["written"]) / (dec["total_ms"] / 1e3)
        out["k_bed_decode"] = {"bytes_read": b["read"], "bytes_written": b["written"], "total_ms": dec["total_ms"], "calls": dec["calls"],
                               "bytes_per_s": rate, "share_of_8TBps_roof": rate / HBM_BYTES_PER_S}
    return out


def bench_shape(n, L, work, reps):
    from eagleeverything_amd import r_api, rcpp_api, synth
    need = 2 * n * L + n * L // 4 + 2 * (2 * n * L + n * L // 2) + (1 << 30)   # table, bed, two output sets, slack
    free = shutil.disk_usage(work).free
    if need > free:
        return {"n": n, "L": L, "skipped": "needs %.1f GB of disk, %.1f GB free" % (need / 1e9, free / 1e9)}
    Mt8 = synth.genotypes_marker_major(n, L, seed=5)
    table, prefix = os.path.join(work, "panel.txt"), os.path.join(work, "panel")
    write_table(table, Mt8)
    bed = synth.write_bed(prefix, Mt8)
    del Mt8
    d_bed, d_txt = os.path.join(work, "out_bed"), os.path.join(work, "out_txt")
    os.makedirs(d_bed, exist_ok=True), os.makedirs(d_txt, exist_ok=True)
    res = {"n": n, "L": L, "input_bytes": {"bed": os.path.getsize(bed), "text": os.path.getsize(table)}, "bed_wall_s": [], "text_wall_s": []}
    for _ in range(reps):
        rcpp_api.drop_cache()
        t0 = time.perf_counter()
        assert r_api.ReadMarker(bed, type="PLINKbed", outdir=d_bed) is not None
        res["bed_wall_s"].append(time.perf_counter() - t0)
        rcpp_api.drop_cache()
        t0 = time.perf_counter()
        assert r_api.ReadMarker(table, type="text", AA=0, AB=1, BB=2, outdir=d_txt) is not None
        res["text_wall_s"].append(time.perf_counter() - t0)
    res["outputs_identical"] = same_outputs(d_bed, d_txt)
    rcpp_api.drop_cache()
    geno = r_api.ReadMarker(bed, type="PLINKbed", outdir=d_bed)
    t0 = time.perf_counter()
    K1 = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 16, np.nan, (n, L))
    res["first_MMt_after_ingest_s"] = time.perf_counter() - t0
    rcpp_api.drop_cache()
    t0 = time.perf_counter()
    K2 = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, 16, np.nan, (n, L))
    res["MMt_after_drop_cache_s"] = time.perf_counter() - t0
    res["MMt_equal"] = bool(np.array_equal(K1, K2))
    rcpp_api.drop_cache()
    for d in (d_txt, d_bed):
        shutil.rmtree(d)
    os.remove(table)
    return res, bed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5000x200000,10000x200000")
    ap.add_argument("--big", default="")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bed_ingest.json"))
    ap.add_argument("--no-kernel-stats", action="store_true")
    ap.add_argument("--child-ingest", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_ingest:
        return child_ingest(a.child_ingest, a.dir)
    from eagleeverything_amd import r_api, rcpp_api, synth
    work = tempfile.mkdtemp(prefix="bench_bed_", dir=a.dir)
    out = {"device": rcpp_api.device_info(), "shapes": [], "hbm_roof_bytes_per_s": HBM_BYTES_PER_S}
    try:
        # warm-up: both routes on a small panel
        wdir = os.path.join(work, "warm")
        os.makedirs(wdir)
        Mw = synth.genotypes_marker_major(500, 3000, seed=1)
        write_table(os.path.join(wdir, "w.txt"), Mw)
        r_api.ReadMarker(synth.write_bed(os.path.join(wdir, "w"), Mw), type="PLINKbed", outdir=wdir)
        r_api.ReadMarker(os.path.join(wdir, "w.txt"), type="text", AA=0, AB=1, BB=2, outdir=wdir)
        rcpp_api.drop_cache()
        shutil.rmtree(wdir)
        first_bed = None
        for shape in a.shapes.split(","):
            n, L = (int(v) for v in shape.split("x"))
            r = bench_shape(n, L, work, a.reps)
            if isinstance(r, tuple):
                r, bed = r
                if first_bed is None:
                    first_bed = (bed, n, L)
                else:
                    for ext in (".bed", ".bim", ".fam"):
                        os.remove(bed[:-4] + ext)
            out["shapes"].append(r)
            print(json.dumps(r), flush=True)
        if first_bed and not a.no_kernel_stats:
            rcpp_api.close_all()
            out["kernel_stats"] = dict(kernel_stats(first_bed[0], work, first_bed[1], first_bed[2]), n=first_bed[1], L=first_bed[2])
            print(json.dumps(out["kernel_stats"]), flush=True)
        out["big"] = {"not_run": "no --big shape was asked for"}
        if a.big:
            n, L = (int(v) for v in a.big.split("x"))
            need = n * L // 4 + 2 * n * L + n * L // 2 + (1 << 30)
            free = shutil.disk_usage(work).free
            if need > free:
                out["big"] = {"n": n, "L": L, "not_run": "needs %.1f GB of disk, %.1f GB free" % (need / 1e9, free / 1e9)}
            else:
                prefix = os.path.join(work, "big")
                for l0 in range(0, L, 100000):   # the panel in marker blocks: .bed rows append
                    blk = synth.genotypes_marker_major(n, min(100000, L - l0), seed=5, first_marker=l0)
                    synth.write_bed(prefix + "_blk", blk)
                    with open(prefix + ".bed", "ab") as f, open(prefix + "_blk.bed", "rb") as g:
                        if l0:
                            g.seek(3)
                        shutil.copyfileobj(g, f)
                    for ext in (".bim", ".fam"):
                        with open(prefix + ext, "a" if (l0 and ext == ".bim") else "w") as f, open(prefix + "_blk" + ext) as g:
                            f.write(g.read())
                d_big = os.path.join(work, "out_big")
                os.makedirs(d_big)
                t0 = time.perf_counter()
                geno = r_api.ReadMarker(prefix, type="PLINKbed", outdir=d_big)
                out["big"] = {"n": n, "L": L, "bed_wall_s": time.perf_counter() - t0, "dims": geno["dim_of_ascii_M"],
                              "input_bytes": os.path.getsize(prefix + ".bed"),
                              "output_bytes": os.path.getsize(geno["asciifileM"]) + os.path.getsize(geno["asciifileMt"])}
            print(json.dumps(out["big"]), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
