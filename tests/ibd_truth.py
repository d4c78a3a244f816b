"""Pairwise IBD-type segments straight from the definitions (include/eagle_hip.h section 1b'''vii, rules 2 to 8) in plain Python loops -- no
bit tricks, no cumulative sums -- and the seeded founder-mosaic panel builder.  Shared by test_ibd_host.py, test_gpu_ibd.py and
test_gpu_bed_ibd.py."""
import numpy as np

DEFAULTS = dict(mode=1, min_snp=200, min_len=0, max_gap=0, merge_min=100)


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


def pieces(chrom, ps, L, max_gap):
    """Rule 3 -> [(first, end, block ordinal)]."""
    out = []
    for b, (a, e) in enumerate(blocks(chrom, L)):
        s = a
        for m in range(a + 1, e):
            if max_gap > 0 and ps[m] - ps[m - 1] > max_gap:
                out.append((s, m, b))
                s = m
        out.append((s, e, b))
    return out


def is_break(gi, gj, ci, cj, mode):
    """Rule 2 for one marker."""
    if not (ci and cj):
        return False
    return gi * gj == -1 if mode == 1 else gi != gj


def pair_candidates(g, called, i, j, pcs, p):
    """Rules 4 and 5 for one pair -> [(s, e, k, block ordinal)] in marker order."""
    out = []
    for a, e, b in pcs:
        runs, m = [], a
        while m < e:                                     # rule 4: the pure runs of the piece
            if is_break(int(g[m, i]), int(g[m, j]), bool(called[m, i]), bool(called[m, j]), p["mode"]):
                m += 1
                continue
            s = m
            while m + 1 < e and not is_break(int(g[m + 1, i]), int(g[m + 1, j]), bool(called[m + 1, i]), bool(called[m + 1, j]), p["mode"]):
                m += 1
            runs.append((s, m))
            m += 1
        eligible = [p["merge_min"] >= 1 and r[1] - r[0] + 1 >= p["merge_min"] for r in runs]
        r = 0
        while r < len(runs):                             # rule 5: the maximal chain that starts at run r
            t = r
            while t + 1 < len(runs) and eligible[t] and eligible[t + 1] and runs[t + 1][0] - runs[t][1] == 2:
                t += 1
            out.append((runs[r][0], runs[t][1], t - r + 1, b))
            r = t + 1
    return out


def ibd_loops(g, called=None, pairs=None, chrom=None, pos=None, **params):
    """Rules 2 to 8 -> (pair int64 (P, 4), seg int32 (S, 6)).  g: int8 (L, n) of -1 / 0 / +1, called: bool (L, n) or None."""
    p = dict(DEFAULTS)
    p.update(params)
    g = np.asarray(g)
    L, n = g.shape
    called = np.ones((L, n), dtype=bool) if called is None else np.asarray(called)
    ps = list(range(L)) if pos is None else [int(x) for x in pos]
    if pairs is None:
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    pcs = pieces(chrom, ps, L, p["max_gap"])
    tab = np.zeros((len(pairs), 4), dtype=np.int64)
    rows = []
    for k, (i, j) in enumerate(pairs):
        i, j = int(i), int(j)
        for s, e, runs, b in pair_candidates(g, called, i, j, pcs, p):
            nsnp, length = e - s + 1, ps[e] - ps[s]
            if nsnp < p["min_snp"] or length < p["min_len"]:
                continue
            rows.append((i, j, s, e, runs - 1, b))
            tab[k, 0] += 1
            tab[k, 1] += nsnp
            tab[k, 2] += length
            tab[k, 3] = max(tab[k, 3], length)
    return tab, np.asarray(rows, dtype=np.int32).reshape(-1, 6)


def mosaic(n, L, F, seed, noise=0.01, miss=0.0):
    """A founder-mosaic panel -> (g int8 (L, n) of -1 / 0 / +1, called bool (L, n)).  F founder genotype columns with a per-marker allele
    frequency between 0.1 and 0.5 and 5 % het; every individual is a mosaic of founder stretches of 20 to 299 markers; `noise` of the
    entries are redrawn from the marker's frequencies, `miss` of them are not called (g = 0 there, as on the ingested image)."""
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.1, 0.5, L)

    def draw(shape):
        hom = np.where(rng.random(shape) < freq[:, None], 1, -1).astype(np.int8)
        return np.where(rng.random(shape) < 0.05, 0, hom).astype(np.int8)
    founders = draw((L, F))
    g = np.zeros((L, n), dtype=np.int8)
    for i in range(n):
        m = 0
        while m < L:
            ln = int(rng.integers(20, 300))
            g[m:m + ln, i] = founders[m:m + ln, int(rng.integers(0, F))]
            m += ln
    redraw = rng.random((L, n)) < noise
    g = np.where(redraw, draw((L, n)), g).astype(np.int8)
    called = rng.random((L, n)) >= miss if miss > 0 else np.ones((L, n), dtype=bool)
    g[~called] = 0
    return g, called
