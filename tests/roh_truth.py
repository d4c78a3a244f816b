"""Runs of homozygosity straight from the definitions (include/eagle_hip.h section 1b'''vi, rules 2 to 7) in plain Python loops -- no
cumulative sums, no shift registers -- and a seeded panel builder.  Shared by test_roh_host.py, test_gpu_roh.py and test_gpu_bed_roh.py."""
import numpy as np

DEFAULTS = dict(w=50, win_het=1, win_miss=5, thr16=3277, min_snp=100, min_len=0, max_gap=0, max_density=0, max_het=-1)


def blocks(chrom, L):
    if chrom is None:
        return [(0, L)]
    out, a = [], 0
    for m in range(1, L):
        if chrom[m] != chrom[m - 1]:
            out.append((a, m))
            a = m
    out.append((a, L))
    return out


def flags_loops(classes, chrom, p):
    """Rules 3 and 4 -> bool (L, n)."""
    L, n = classes.shape
    w = p["w"]
    flagged = np.zeros((L, n), dtype=bool)
    for a, e in blocks(chrom, L):
        for i in range(n):
            col = classes[a:e, i]
            for m in range(a, e):
                cover = hom = 0
                for s in range(m - w + 1, m + 1):
                    if s < a or s + w > e:
                        continue
                    cover += 1
                    win = col[s - a:s - a + w]
                    if int((win == 1).sum()) <= p["win_het"] and int((win == 2).sum()) <= p["win_miss"]:
                        hom += 1
                flagged[m, i] = hom >= 1 and hom * 65536 >= p["thr16"] * cover
    return flagged


def roh_loops(classes, chrom=None, pos=None, **params):
    """Rules 2 to 7 -> (ind int64 (n, 4), seg int32 (S, 6))."""
    p = dict(DEFAULTS)
    p.update(params)
    classes = np.asarray(classes)
    L, n = classes.shape
    ps = list(range(L)) if pos is None else [int(x) for x in pos]
    flagged = flags_loops(classes, chrom, p)
    blks = blocks(chrom, L)
    rows = []
    ind = np.zeros((n, 4), dtype=np.int64)
    for i in range(n):
        for b, (a, e) in enumerate(blks):
            m = a
            while m < e:
                if not flagged[m, i]:
                    m += 1
                    continue
                s = m
                while m + 1 < e and flagged[m + 1, i] and not (p["max_gap"] > 0 and ps[m + 1] - ps[m] > p["max_gap"]):
                    m += 1
                last = m
                m += 1
                nsnp, length = last - s + 1, ps[last] - ps[s]
                nhet = int((classes[s:last + 1, i] == 1).sum())
                nmiss = int((classes[s:last + 1, i] == 2).sum())
                if nsnp < p["min_snp"] or length < p["min_len"]:
                    continue
                if p["max_density"] != 0 and length > p["max_density"] * nsnp:
                    continue
                if p["max_het"] >= 0 and nhet > p["max_het"]:
                    continue
                rows.append((i, s, last, nhet, nmiss, b))
                ind[i, 0] += 1
                ind[i, 1] += nsnp
                ind[i, 2] += length
                ind[i, 3] = max(ind[i, 3], length)
    return ind, np.asarray(rows, dtype=np.int32).reshape(-1, 6)


def planted_panel(n, L, seed, planted, het_rate=0.5, miss_rate=0.0):
    """classes uint8 (L, n): a background of het rate `het_rate` (and missing calls at miss_rate), with the fully homozygous segments
    planted = [(individual, first, last), ...] written over it (no het, no missing call inside)."""
    rng = np.random.default_rng(seed)
    cl = (rng.random((L, n)) < het_rate).astype(np.uint8)
    if miss_rate > 0:
        cl[rng.random((L, n)) < miss_rate] = 2
    for i, s, e in planted:
        cl[s:e + 1, i] = 0
    return cl


def mt8_of_classes(classes, seed=0):
    """An int8 image (L, n) with the given hom / het classes (no class 2): hom -> -1 or +1 at random, het -> 0."""
    rng = np.random.default_rng(seed)
    cl = np.asarray(classes)
    assert cl.max() <= 1
    sign = np.where(rng.random(cl.shape) < 0.5, -1, 1).astype(np.int8)
    return np.where(cl == 0, sign, 0).astype(np.int8)


def bed_codes_of_classes(classes, seed=0):
    """2-bit .bed codes (L, n) with the given classes: hom -> 0 or 3 at random, het -> 2, miss -> 1."""
    rng = np.random.default_rng(seed)
    cl = np.asarray(classes)
    homc = np.where(rng.random(cl.shape) < 0.5, 0, 3).astype(np.uint8)
    return np.where(cl == 0, homc, np.where(cl == 1, 2, 1)).astype(np.uint8)
