"""The transmission disequilibrium test straight from the definition (include/eagle_hip.h section 1b''''viii, rules 1 to 5) in plain Python
loops over ALLELE CHOICES -- no bit planes, no matrix products -- with the flips on Python ints, and the panels the TDT tests share.
Shared by test_tdt_host.py, test_gpu_tdt.py and test_gpu_bed_tdt.py."""
import itertools

import numpy as np

import mendel_truth as M

MASK64 = (1 << 64) - 1


def transmissions(gc, cc, gf, cf, gm, cm):
    """One trio at one marker -> (PT, PU, MT, MU, W, complete, het father, het mother), all 0 / 1.  The trio is complete when all three are
    called and some choice of one allele from each parent gives the child's genotype.  A het parent whose transmitted allele is the same in
    every consistent choice counts to PT / MT (allele A2) or PU / MU (allele A1); where both alleles occur (het x het -> het) the trio
    counts to W."""
    if not (cc and cf and cm):
        return (0,) * 8
    fa, ma, want = M.ALLELES[int(gf)], M.ALLELES[int(gm)], tuple(sorted(M.ALLELES[int(gc)]))
    choices = [(a, b) for a in fa for b in ma if tuple(sorted((a, b))) == want]
    if not choices:
        return (0,) * 8                                  # a Mendel error
    hf, hm = int(gf) == 0, int(gm) == 0
    by_f, by_m = {a for a, _ in choices}, {b for _, b in choices}
    pt = int(hf and by_f == {1})
    pu = int(hf and by_f == {0})
    mt = int(hm and by_m == {1})
    mu = int(hm and by_m == {0})
    w = int(hf and hm and by_f == {0, 1} and by_m == {0, 1})
    assert not (hf and by_f == {0, 1}) or w, "a het father passes both alleles only in het x het -> het"
    assert not (hm and by_m == {0, 1}) or w
    return pt, pu, mt, mu, w, 1, int(hf), int(hm)


def triple_table():
    """{(child, father, mother) code triple: transmissions(...)} over all 64 triples of (hom A1, het, hom A2, not called)."""
    return {t: transmissions(M.G_OF_CODE[t[0]], t[0] != 3, M.G_OF_CODE[t[1]], t[1] != 3, M.G_OF_CODE[t[2]], t[2] != 3)
            for t in itertools.product(M.CODES, repeat=3)}


def informative_triples():
    """The called code triples with an informative het parent: 11 of the 27."""
    return [t for t, v in sorted(triple_table().items()) if v[6] + v[7] > 0]


def mix32(seed, r, j):
    """The 32-bit splitmix64 value of rule 4 of section 1b''''vi at counter = r 2^16 + j + 1, on Python ints."""
    z = (seed + ((r << 16) + j + 1) * 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z >> 32


def sign(seed, r, phi):
    return -1 if mix32(seed, r, phi) >> 31 else 1


def families(trios):
    """Rule 5 without family ids: the smallest list position with the same (father, mother)."""
    out = []
    for k, (_, f, m) in enumerate(trios):
        out.append(next(j for j, (_, f2, m2) in enumerate(trios) if (f2, m2) == (f, m)))
    return out


def key(d, v):
    return float(d * d) / float(v) if v else 0.0         # d d < 2^53: float() of the exact product is the rounded product


def tdt_loops(g, called, trios, family=None, seed=0, first=1, R=0):
    """Rules 1 to 5 -> the dict of rcpp_api.tdt: trio (T, 6), marker (L, 5), key_obs, count1, maxkey, argmax."""
    g = np.asarray(g)
    L, n = g.shape
    called = np.ones((L, n), dtype=bool) if called is None else np.asarray(called)
    trios = [tuple(int(v) for v in t) for t in np.asarray(trios).tolist()]
    T = len(trios)
    tab = np.zeros((T, 6), dtype=np.int32)
    marker = [[0] * 5 for _ in range(L)]
    d = [[0] * T for _ in range(L)]
    for k, (c, f, m) in enumerate(trios):
        (gc, cc), (gf, cf), (gm, cm) = M.column(g, called, c, L), M.column(g, called, f, L), M.column(g, called, m, L)
        for x in range(L):
            pt, pu, mt, mu, w, comp, hf, hm = transmissions(gc[x], cc[x], gf[x], cf[x], gm[x], cm[x])
            tab[k] += (comp, hf, hm, pt + mt + w, pu + mu + w, w)
            for j, v in enumerate((pt, pu, mt, mu, w)):
                marker[x][j] += v
            d[x][k] = pt + mt - pu - mu
    tu = [(r[0] + r[2] + r[4], r[1] + r[3] + r[4]) for r in marker]
    d_obs, V = [t - u for t, u in tu], [t + u for t, u in tu]
    assert d_obs == [sum(row) for row in d]
    out = {"trio": tab, "marker": np.asarray(marker, dtype=np.int32).reshape(L, 5),
           "key_obs": np.asarray([key(a, v) for a, v in zip(d_obs, V)], dtype=np.float64), "count1": np.zeros(L, dtype=np.int32),
           "maxkey": np.zeros(R, dtype=np.float64), "argmax": np.zeros(R, dtype=np.int32)}
    if R >= 1:
        fam = families(trios) if family is None else [int(v) for v in family]
        for q in range(R):
            s = [sign(int(seed), first + q, phi) for phi in fam]
            dr = [sum(sk * dk for sk, dk in zip(s, row)) for row in d]
            ks = [key(a, v) for a, v in zip(dr, V)]
            for x in range(L):
                out["count1"][x] += abs(dr[x]) >= abs(d_obs[x])
            out["maxkey"][q] = max(ks)
            out["argmax"][q] = ks.index(max(ks))
    return out


def same(got, want, what=""):
    """Every output of two TDT dicts agrees word for word."""
    for k in ("trio", "marker", "key_obs", "count1", "maxkey", "argmax"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5].tolist(), a[a != b][:5], b[a != b][:5])


def edge_markers(L):
    """Bits 0 and 63 of every word, and the last marker."""
    return sorted({x for x in range(L) if x % 64 in (0, 63)} | {L - 1})


def kinds_panel(L, hide, seed=0):
    """81 individuals in 27 trios (3 k + 2, 3 k, 3 k + 1) over random genotypes, then three more individuals; trio k < 11 gets informative
    triple k and trio 11 + k the Mendel error triple k, at every edge marker.  hide: the not-called codes of the error triples stay not
    called (the .bed route); else they are hets (the image) -> (g, called, trios)."""
    rng = np.random.default_rng(1000 + L + seed)
    n = 84
    g = rng.integers(-1, 2, (L, n)).astype(np.int8)
    called = np.ones((L, n), dtype=bool)
    trios = np.asarray([(3 * k + 2, 3 * k, 3 * k + 1) for k in range(27)], dtype=np.int32)
    kinds = informative_triples() + M.error_triples()
    assert len(kinds) == 27
    for k, trio in enumerate(trios.tolist()):
        for x in edge_markers(L):
            M.plant(g, called, trio, x, kinds[k])
    if not hide:
        called[:] = True
    g[~called] = 0
    return g, called, trios
