"""Times eagle_vcf_to_bed (include/eagle_hip.h section 1b-vcf) beside eagle_bed_marker_counts on the .bed file it wrote, in one run:

  vcf_ms     eagle_vcf_to_bed, the whole call from a warm page cache: pread of the text in windows, the host's newline scan and
             fixed-field parse, the upload, k_vcf_fields and k_vcf_pack, the rows back and written behind, .bim and .fam
  counts_ms  eagle_bed_marker_counts on the resulting .bed file: the yardstick -- a sixteenth of the bytes or less through the same ring

The VCF is synthetic, made with numpy byte operations in blocks of lines: n samples x L biallelic SNP lines, FORMAT GT:DP, the fields
drawn from forms of 5 to 8 bytes ("0/0:9" ... "0|1:123"), 5 % of them "./.:0".  Before timing, the first rows of the .bed file are
compared with r_api.vcf_to_bed_host on the head of the text.  The two calls are alternated rep by rep, medians reported.  Wall-clock
times of whole calls, file reads from the page cache and file writes included; no kernel is timed on its own -- a kernel trace is a
run of its own (rocprofv3 --kernel-trace --stats -- python tools/vcf_timing.py 4096 8192 2 /tmp/x.json).

    python tools/vcf_timing.py [n] [L] [reps] [out.json]       (default 4096 65536 7 profiles/r28_vcf.json)
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = [b"0/0:9", b"0/1:14", b"1/1:8", b"0|1:123", b"1|1:31", b"0/0:27", b"1|0:6", b"./.:0"]
PROBS = [0.30, 0.15, 0.15, 0.10, 0.10, 0.10, 0.05, 0.05]


def write_vcf(path, n, L, seed=28, block=512):
    """The synthetic VCF -> its size in bytes."""
    rng = np.random.default_rng(seed)
    width = max(len(f) for f in FORMS)
    table = np.zeros((len(FORMS), width), dtype=np.uint8)
    for k, f in enumerate(FORMS):
        table[k, :len(f)] = np.frombuffer(f, dtype=np.uint8)
    flen = np.array([len(f) for f in FORMS], dtype=np.int64)
    pre = np.frombuffer(b"1\t100000000\t.\tA\tC\t.\tPASS\t.\tGT:DP\t", dtype=np.uint8)      # POS is overwritten: nine digits
    P = pre.size
    with open(path, "wb") as f:
        f.write(b"##fileformat=VCFv4.2\n##source=tools/vcf_timing.py\n")
        f.write(b"\t".join([b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO", b"FORMAT"] + [b"s%d" % i for i in range(n)]) + b"\n")
        for r0 in range(0, L, block):
            rows = min(block, L - r0)
            form = rng.choice(len(FORMS), size=(rows, n), p=PROBS).astype(np.uint8)
            lens = flen[form] + 1                                              # the field and its tab (the newline in the last column)
            lens[:, 0] += P
            off = np.cumsum(lens.ravel()).reshape(rows, n) - lens              # where every field's span starts
            out = np.empty(int(off[-1, -1] + lens[-1, -1]), dtype=np.uint8)
            start = off[:, 0].copy()                                           # line starts
            off[:, 0] += P
            lens[:, 0] -= P
            line = np.broadcast_to(pre, (rows, P)).copy()
            pos = 100000000 + 100 * (r0 + np.arange(rows, dtype=np.int64))
            for d in range(9):
                line[:, 2 + d] = 48 + (pos // 10 ** (8 - d)) % 10
            out[start[:, None] + np.arange(P)[None, :]] = line
            fo, ff = off.ravel(), form.ravel()
            for c in range(width):
                m = flen[ff] > c
                out[fo[m] + c] = table[ff[m], c]
            sep = np.full((rows, n), 9, dtype=np.uint8)
            sep[:, -1] = 10
            out[fo + flen[ff]] = sep.ravel()
            f.write(out.tobytes())
    return os.path.getsize(path)


def main():
    arg = lambda i, d, f: f(sys.argv[i]) if len(sys.argv) > i else d
    n, L, reps = arg(1, 4096, int), arg(2, 65536, int), arg(3, 7, int)
    out_path = arg(4, os.path.join(ROOT, "profiles", "r28_vcf.json"), str)
    import torch
    from eagleeverything_amd import r_api, rcpp_api
    with tempfile.TemporaryDirectory() as d:
        vcf, prefix = os.path.join(d, "synth.vcf"), os.path.join(d, "out")
        t0 = time.perf_counter()
        text_bytes = write_vcf(vcf, n, L)
        make_s = time.perf_counter() - t0
        res = rcpp_api.vcf_to_bed(vcf, prefix)                                  # warm-up: the page cache, the staging buffers
        assert res["dims"] == [n, L] and res["counts"]["kept"] == L and res["counts"]["malformed"] == 0
        head_lines = min(L, 8)
        with open(vcf, "rb") as f:
            head = b"".join(f.readline() for _ in range(3 + head_lines))
        hbed = r_api.vcf_to_bed_host(head)[0]
        with open(res["bed"], "rb") as f:
            assert f.read(len(hbed)) == hbed, "eagle_vcf_to_bed differs from the host restatement"
        counts = rcpp_api.bed_marker_counts(res["bed"], (n, L))
        assert int(counts[:, 3].sum()) == res["counts"]["missing"]
        fns = [lambda: rcpp_api.vcf_to_bed(vcf, prefix), lambda: rcpp_api.bed_marker_counts(res["bed"], (n, L))]
        names = ["vcf", "counts"]
        ts = [[] for _ in fns]
        for _ in range(reps):
            for i, fn in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts[i].append((time.perf_counter() - t0) * 1e3)
        bed_bytes = os.path.getsize(res["bed"])
    out = {"n": n, "L": L, "reps": reps, "text_bytes": text_bytes, "bed_bytes": bed_bytes, "missing": res["counts"]["missing"],
           "make_vcf_s": make_s, "device": torch.cuda.get_device_name(0),
           "what": "wall-clock times of whole calls from a warm page cache (file reads and writes included), the two calls alternated, medians",
           "not_timed": "the kernels on their own (no kernel trace taken in this run), a cold page cache, compressed input, chunk_bytes other than 0"}
    for name, t in zip(names, ts):
        out.update({name + "_ms": float(np.median(t)), name + "_ms_min": float(np.min(t)), name + "_ms_max": float(np.max(t))})
    out["vcf_text_GBps"] = text_bytes / (out["vcf_ms"] * 1e-3) / 1e9
    out["counts_bed_GBps"] = bed_bytes / (out["counts_ms"] * 1e-3) / 1e9
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
