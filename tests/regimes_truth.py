"""Builders and restated launch arithmetic for tests/test_gpu_regimes.py: the panels, tables and matrices of the cases that run the
n-sized kernels at every row-length regime and at their capacities, and the per-row restatements used where a whole-matrix restatement
is too heavy at the shape.  CPU only; tests/test_regimes_host.py pins every function here to r_api's restatements or to plain loops,
and the constants to the source text of the kernels."""
import numpy as np

HEAD = b"\x6c\x1b\x01"

# csrc/eagle_impute.hip
IMP_STAGE_BYTES = 245760 // 4             # EAGLE_IMPUTE_MAX_N / 4
IMP_MAX_ROWS = 256
IMP_WALK_RB = 256                         # rb >= 256: a thread walks the byte columns tid, tid + 256, ... of every row
KNN_THREADS = 256
# csrc/eagle_ldknn.hip
LDK_THREADS = 512
# csrc/eagle_mendel.hip, csrc/eagle_ingest.cpp
GRID_Y = 65535


def row_bytes(n):
    return (n + 3) // 4


def imp_rows_per_block(rb):
    """imp_rows_per_block of csrc/eagle_impute.hip."""
    return max(1, min(IMP_STAGE_BYTES // rb, IMP_MAX_ROWS, max(1, 16384 // rb)))


def imp_rows_regime(rb):
    """Which term of imp_rows_per_block decides: "256" (rb <= 64), "16384/rb" (64 < rb <= 16384), "1" (rb > 16384: 16384 / rb is 0)."""
    return "256" if rb <= 64 else ("16384/rb" if rb <= 16384 else "1")


def ldk_lds_bytes(n):
    """ldk_lds_bytes of csrc/eagle_ldknn.hip: three word arrays of pad4(n) dwords and two copies of the target row in whole dwords."""
    return (3 * ((n + 3) // 4 * 4) + 2 * ((row_bytes(n) + 3) // 4)) * 4


def knn_lds_bytes(n):
    return 4 * n


def trips(count, step):
    """Trips of `for (x = tid; x < count; x += step)` made by thread 0."""
    return (count + step - 1) // step


def parentage_parts(ns, nd):
    """eagle_parentage_parts of csrc/eagle_mendel.hip (PAR_SB * PAR_WAVES = 16 sires, 64 dams a workgroup)."""
    return ((max(ns, 1) + 15) // 16) * ((max(nd, 1) + 63) // 64)


def parentage_chunk(n_o, ns, nd):
    """parentage_chunk of csrc/eagle_ingest.cpp."""
    return max(1, min(n_o, GRID_Y, (1 << 28) // (24 * parentage_parts(ns, nd))))


# ------------------------------------------------------------------------------------------------ .bed panels
def codes_panel(n, L, seed, rate, dense=None, full=None, empty=None):
    """uint8 (L, n) 2-bit codes (0 hom A1, 1 missing, 2 het, 3 hom A2): genotypes at random with `rate` missing; marker `dense` has 40 %
    missing (neighbours that are themselves missing), marker `full` has no missing call, marker `empty` has every call missing."""
    rng = np.random.default_rng(seed)
    codes = np.array([0, 2, 3], dtype=np.uint8)[rng.integers(0, 3, size=(L, n))]
    codes[rng.random((L, n)) < rate] = 1
    if dense is not None:
        codes[dense, rng.random(n) < 0.4] = 1
    if full is not None:
        row = codes[full]
        row[row == 1] = 2
    if empty is not None:
        codes[empty] = 1
    return codes


def cluster_panel(n, L, seed, rate, founders=8, noise=0.03):
    """(codes, full): uint8 (L, n) codes of individuals that copy one of `founders` random founders each but for 3 % of their genotypes,
    `rate` of the codes missing, and the same without the missing codes.  The individuals nearest over any markers are those of one's own
    founder, so what is imputed depends on WHICH neighbours vote: on independent genotypes the rounded mean of 64 voters is a het whoever
    they are."""
    rng = np.random.default_rng(seed)
    lut = np.array([0, 2, 3], dtype=np.uint8)
    full = lut[rng.integers(0, 3, size=(L, founders))][:, rng.integers(0, founders, size=n)]
    redraw = rng.random((L, n)) < noise
    full[redraw] = lut[rng.integers(0, 3, size=int(redraw.sum()))]
    codes = full.copy()
    codes[rng.random((L, n)) < rate] = 1
    return codes, full


def write_codes(path, codes, garbage_pad=True):
    """The SNP-major .bed file of `codes` at `path` (no .bim, no .fam: the eagle_bed_* entry points take the dims).  garbage_pad: the unused
    bit pairs of every row's last byte hold 01 (missing), 11 and 10 -- never individuals."""
    from eagleeverything_amd import r_api
    rows = r_api.pack_bed_codes(codes)
    n = codes.shape[1]
    if garbage_pad and n % 4:
        rows[:, -1] |= (0b10110101 << (2 * (n % 4))) & 0xff
    with open(path, "wb") as f:
        f.write(HEAD)
        f.write(rows.tobytes())
    return path


def neighbour_table(n, K, seed):
    """int32 (n, K) of knn_rows' shape without the cost of distances: others at random (never i itself), every third row with a -1 tail
    from a random column on, row 1 all -1 (when n > 1)."""
    rng = np.random.default_rng(seed)
    if n == 1:
        return np.full((1, K), -1, dtype=np.int32)
    p = rng.integers(0, n - 1, size=(n, K))
    nbr = (p + (p >= np.arange(n)[:, None])).astype(np.int32)
    cut = rng.integers(0, K + 1, size=n)
    tail = (np.arange(K)[None, :] >= cut[:, None]) & (np.arange(n) % 3 == 0)[:, None]
    nbr[tail] = -1
    nbr[1] = -1
    return nbr


_DOSAGE_OF_CODE = np.array([0, 0, 1, 2], dtype=np.int64)
_CODE_OF_DOSAGE = np.array([0, 2, 3], dtype=np.uint8)


def impute_knn_sparse(codes, nbr, k, min_votes):
    """r_api.impute_knn_host's result, computed over the missing genotypes only (the host restatement walks all L n genotypes K times,
    seconds at K = 256): for a missing (m, i) the first k entries of nbr[i] that are >= 0 and called at m vote, the dosage is
    (2 s + c) // (2 c), and with fewer than min_votes voters the marker's own mean gives it (heterozygous without a call)."""
    from eagleeverything_amd import r_api
    codes = np.asarray(codes, dtype=np.uint8)
    nbr = np.asarray(nbr, dtype=np.int64)
    L, n = codes.shape
    out = codes.copy()
    counts = np.zeros((L, 2), dtype=np.int32)
    called = (codes != 1).sum(axis=1)
    dose = _DOSAGE_OF_CODE[codes].sum(axis=1)                                 # code 1 has dosage 0 in the table
    fb = np.where(called > 0, _CODE_OF_DOSAGE[(2 * dose + called) // np.maximum(2 * called, 1)], 2).astype(np.uint8)
    mm, ii = np.nonzero(codes == 1)
    for a in range(0, mm.size, 1 << 15):
        m, i = mm[a:a + (1 << 15)], ii[a:a + (1 << 15)]
        lst = nbr[i]                                                          # (missing, K)
        cj = codes[m[:, None], np.maximum(lst, 0)]
        can = (lst >= 0) & (cj != 1)
        vote = can & (np.cumsum(can, axis=1) <= k)
        c = vote.sum(axis=1)
        s = np.where(vote, _DOSAGE_OF_CODE[cj], 0).sum(axis=1)
        by_vote = c >= min_votes
        out[m, i] = np.where(by_vote, _CODE_OF_DOSAGE[np.where(by_vote, (2 * s + c) // np.maximum(2 * c, 1), 0)], fb[m])
        np.add.at(counts[:, 0], m[by_vote], 1)
        np.add.at(counts[:, 1], m[~by_vote], 1)
    return r_api.pack_bed_codes(out), counts


def ld_neighbours(L, reach=16):
    """int32 (L, 2 reach): the markers m - 1, m + 1, m - 2, m + 2, ... m - reach, m + reach of the panel, those outside it dropped and -1
    behind the rest: the first l columns are the l nearest."""
    part = np.full((L, 2 * reach), -1, dtype=np.int32)
    for m in range(L):
        near = [j for o in range(1, reach + 1) for j in (m - o, m + o) if 0 <= j < L]
        part[m, :len(near)] = near
    return part


# ------------------------------------------------------------------------------------------------ neighbour tables at large n
def _mix(x, mult):
    x = (np.asarray(x).astype(np.uint32) + np.uint32(0x7f4a7c15)) * np.uint32(mult)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x2c1b3c6d)
    x ^= x >> np.uint32(13)
    return x


def hash_rows(rows, n, salt=0, out=None):
    """uint32 (len(rows), n): a hash of (i, j) in one pass over the matrix, a_i + b_j mod 2^32 of two mixed vectors; its top bits are used.
    out: where to write it (the builders of whole matrices fill them band by band in place)."""
    return np.add.outer(_mix(rows, 0x9e3779b1 + 2 * salt), _mix(np.arange(n), 0x85ebca77 + 2 * salt), out=out)


def dist_rows(rows, n, out=None):
    """Rows `rows` of the uint32 (n, n) matrix of the knn_rows_dist cases.  An entry is the top 12 bits of the hash -- about n / 4096
    columns share every value of a row, so the smaller-j rule decides inside every neighbour list -- with 0xffff0000 set in the columns
    j % 3 == 2 (the top of the key's high dword) and 0xfffffffe (bed_sample_ibs' no-overlap value) in the columns j % 64 == (i // 64) % 64.
    Rows i % 4096 == 1 hold one value everywhere (index order alone), rows i % 4096 == 2 only large values, rows i % 4096 == 3 are
    0xfffffffe but for one entry in 128."""
    rows = np.asarray(rows, dtype=np.int64)
    v = hash_rows(rows, n, out=out)
    v >>= np.uint32(20)
    v |= np.where(np.arange(n) % 3 == 2, np.uint32(0xffff0000), np.uint32(0))[None, :]
    offs = (rows >> 6) % 64
    for off in np.unique(offs).tolist():
        v[np.flatnonzero(offs == off)[:, None], np.arange(off, n, 64)[None, :]] = 0xfffffffe
    kind = rows % 4096
    v[kind == 1] = 7
    v[kind == 2] |= np.uint32(0xffff0000)
    for r in np.flatnonzero(kind == 3).tolist():
        v[r] = np.where(np.arange(n) % 128 == 5, v[r] & np.uint32(0xfff), np.uint32(0xfffffffe))
    return v


def dist_matrix(n, band=2048):
    out = np.empty((n, n), dtype=np.uint32)
    for r0 in range(0, n, band):
        dist_rows(np.arange(r0, min(n, r0 + band)), n, out=out[r0:r0 + band])
    return out


def ibs_rows(rows, n, out=(None, None)):
    """Rows `rows` of the (ibs0, hethet) int32 (n, n) pair of the knn_rows case: ibs0 in [0, 64), hethet in [0, 16) off the diagonal and
    h_i = 30 + i % 32 on it, so d = 4 ibs0 + h_i + h_j - 2 hethet lies in [30, 376): ties everywhere."""
    rows = np.asarray(rows, dtype=np.int64)
    ibs0, hethet = hash_rows(rows, n, out=out[0]), hash_rows(rows, n, salt=1, out=out[1])
    ibs0 >>= np.uint32(26)
    hethet >>= np.uint32(28)
    ibs0, hethet = ibs0.view(np.int32), hethet.view(np.int32)
    k = np.arange(rows.size)
    ibs0[k, rows] = 0
    hethet[k, rows] = 30 + rows % 32
    return ibs0, hethet


def ibs_matrices(n, band=2048):
    ibs0, hethet = np.empty((n, n), dtype=np.uint32), np.empty((n, n), dtype=np.uint32)
    for r0 in range(0, n, band):
        ibs_rows(np.arange(r0, min(n, r0 + band)), n, out=(ibs0[r0:r0 + band], hethet[r0:r0 + band]))
    return ibs0.view(np.int32), hethet.view(np.int32)


def knn_row(d_row, i, K):
    """Row i of r_api.knn_rows_host from row i of the distances alone (uint32, or int32 read as uint32): the min(K, n - 1) columns j != i
    with the smallest keys (uint64)d_ij << 32 | j in increasing order, then -1."""
    d = np.ascontiguousarray(d_row).view(np.uint32) if np.asarray(d_row).dtype == np.int32 else np.asarray(d_row, dtype=np.uint32)
    n = d.size
    keys = (d.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    keys = np.delete(keys, i)
    keff = min(K, n - 1)
    out = np.full(K, -1, dtype=np.int32)
    out[:keff] = (np.sort(keys)[:keff] & np.uint64(0xffffffff)).astype(np.int32)
    return out


def sampled_rows(n, count=512, seed=0):
    """`count` rows (all of them when n <= count): 0, n - 1, three around every multiple of 4,096 (where dist_rows plants its rows), the
    rest at random from a fixed seed."""
    if n <= count:
        return np.arange(n)
    fixed = {0, n - 1}
    for base in range(0, n, 4096):
        fixed.update(x for x in range(base - 1, base + 4) if 0 <= x < n)
    rng = np.random.default_rng(seed)
    rest = [x for x in rng.permutation(n).tolist() if x not in fixed][:count - len(fixed)]
    return np.array(sorted(fixed | set(rest)), dtype=np.int64)


# ------------------------------------------------------------------------------------------------ pedigrees
def children(g_par, pairs, seed):
    """int8 (L, c): a child for every row (sire column, dam column) of `pairs` among the columns of g_par (int8 (L, p), -1 / 0 / +1).  A
    child takes one allele of each parent (a het parent passes either), so its true pair has no Mendel error."""
    rng = np.random.default_rng(seed)
    pairs = np.asarray(pairs, dtype=np.int64)

    def allele(cols):
        g = g_par[:, cols]
        return np.where(g == 0, rng.integers(0, 2, size=g.shape), (g + 1) // 2)
    return (allele(pairs[:, 0]) + allele(pairs[:, 1]) - 1).astype(np.int8)
