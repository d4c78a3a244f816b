"""Mendel errors and parentage assignment straight from the definitions (include/eagle_hip.h section 1b'''viii, rules 3 to 6) in plain
Python loops over ALLELE SETS -- no bit planes, no matrix products -- and the seeded pedigree simulator.  Shared by test_mendel_host.py,
test_gpu_mendel.py and test_gpu_bed_mendel.py."""
import itertools

import numpy as np

CODES = (0, 1, 2, 3)                                     # hom A1, het, hom A2, not called
G_OF_CODE = (-1, 0, 1, 0)                                # the genotype value of a code (a not-called entry holds 0, as on the image)
ALLELES = {-1: (0, 0), 0: (0, 1), 1: (1, 1)}             # genotype value -> its two alleles (0 = A1, 1 = A2)


def gametes(g, called):
    """The alleles a parent can pass: those of its genotype, or either when it is not called / unknown."""
    return set(ALLELES[int(g)]) if called else {0, 1}


def is_error(gc, cc, gf, cf, gm, cm):
    """Rule 3 for one marker: the child is called and no choice of one allele from each parent gives its genotype."""
    if not cc:
        return False
    want = tuple(sorted(ALLELES[int(gc)]))
    return not any(tuple(sorted((a, b))) == want for a in gametes(gf, cf) for b in gametes(gm, cm))


def error_triples():
    """The (child, father, mother) code triples that are errors, by brute force over the 64."""
    return [t for t in itertools.product(CODES, repeat=3)
            if is_error(G_OF_CODE[t[0]], t[0] != 3, G_OF_CODE[t[1]], t[1] != 3, G_OF_CODE[t[2]], t[2] != 3)]


def column(g, called, i, L):
    """Genotypes and calls of individual i; -1 is the unknown parent: called nowhere."""
    if i < 0:
        return [0] * L, [False] * L
    return [int(x) for x in g[:, i]], [bool(x) for x in called[:, i]]


def trio_counts(g, called, c, f, m):
    """Rule 4 for one trio -> ((n_cf, e_cf, n_cm, e_cm, n_trio, e), the markers with an error)."""
    L = g.shape[0]
    (gc, cc), (gf, cf), (gm, cm) = column(g, called, c, L), column(g, called, f, L), column(g, called, m, L)
    n_cf = e_cf = n_cm = e_cm = n_trio = 0
    errs = []
    for x in range(L):
        n_cf += cc[x] and cf[x]
        n_cm += cc[x] and cm[x]
        n_trio += cc[x] and cf[x] and cm[x]
        e_cf += cc[x] and cf[x] and gc[x] * gf[x] == -1
        e_cm += cc[x] and cm[x] and gc[x] * gm[x] == -1
        if is_error(gc[x], cc[x], gf[x], cf[x], gm[x], cm[x]):
            errs.append(x)
    return (n_cf, e_cf, n_cm, e_cm, n_trio, len(errs)), errs


def mendel_loops(g, called, trios):
    """Rules 3 to 5 -> (trio int32 (T, 6), marker int32 (L))."""
    g = np.asarray(g)
    L, n = g.shape
    called = np.ones((L, n), dtype=bool) if called is None else np.asarray(called)
    tab = np.zeros((len(trios), 6), dtype=np.int32)
    marker = np.zeros(L, dtype=np.int32)
    for k, (c, f, m) in enumerate(trios):
        tab[k], errs = trio_counts(g, called, int(c), int(f), int(m))
        for x in errs:
            marker[x] += 1
    return tab, marker


def parentage_loops(g, called, offspring, sires, dams, min_overlap=1, allow_self=False):
    """Rule 6 -> int32 (n_o, 2, 4): every candidate of every offspring, one trio at a time."""
    g = np.asarray(g)
    L, n = g.shape
    called = np.ones((L, n), dtype=bool) if called is None else np.asarray(called)
    sl = [int(s) for s in sires] if sires is not None and len(sires) else [-1]
    dl = [int(d) for d in dams] if dams is not None and len(dams) else [-1]
    best = np.full((len(offspring), 2, 4), -1, dtype=np.int32)
    for k, c in enumerate(int(c) for c in offspring):
        cands = []
        for si, s in enumerate(sl):
            for di, d in enumerate(dl):
                if s == c or d == c or (s == d and s >= 0 and not allow_self):
                    continue
                (n_cf, _, n_cm, _, n_trio, e), _ = trio_counts(g, called, c, s, d)
                overlap = n_trio if s >= 0 and d >= 0 else (n_cf if s >= 0 else n_cm)    # single-parent assignment: the known one
                if overlap >= min_overlap:
                    cands.append((e, si * len(dl) + di, s, d, overlap))
        cands.sort()
        for r, (e, _, s, d, overlap) in enumerate(cands[:2]):
            best[k, r] = (s, d, e, overlap)
    return best


def pedigree(founders, children, L, seed, miss=0.0):
    """A simulated pedigree -> (g int8 (L, n), called bool (L, n), trios int32 (children, 3)): `founders` individuals drawn at random
    (allele frequencies 0.2 .. 0.8), the first half sires and the second half dams; every child draws one allele per marker from a sire
    and one from a dam chosen at random among the founders and the earlier children of their half -- so later generations have
    non-founder parents -- and the child joins the sires (even child number) or the dams.  `miss` of the entries are not called (g = 0
    there).  No Mendel error anywhere before the mask; the mask only hides genotypes."""
    rng = np.random.default_rng(seed)
    n = founders + children
    freq = rng.uniform(0.2, 0.8, L)
    hap = np.zeros((2, L, n), dtype=np.int8)
    hap[:, :, :founders] = rng.random((2, L, founders)) < freq[None, :, None]
    sires, dams = list(range(founders // 2)), list(range(founders // 2, founders))
    trios = []
    for k in range(children):
        c = founders + k
        f, m = int(rng.choice(sires)), int(rng.choice(dams))
        for h, p in enumerate((f, m)):
            pick = rng.integers(0, 2, L)
            hap[h, :, c] = np.where(pick == 0, hap[0, :, p], hap[1, :, p])
        trios.append((c, f, m))
        (sires if k % 2 == 0 else dams).append(c)
    g = (hap[0] + hap[1] - 1).astype(np.int8)
    called = rng.random((L, n)) >= miss if miss > 0 else np.ones((L, n), dtype=bool)
    g[~called] = 0
    return g, called, np.asarray(trios, dtype=np.int32).reshape(-1, 3)


def plant(g, called, trio, x, triple):
    """Sets the codes of (child, father, mother) at marker x to a code triple; an unknown parent is left out."""
    for i, code in zip(trio, triple):
        if int(i) >= 0:
            g[x, int(i)] = G_OF_CODE[code]
            called[x, int(i)] = code != 3
