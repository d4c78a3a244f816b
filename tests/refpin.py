"""Shared pieces of the reference pinning (not a conftest): the inputs that tests/golden/make_ref_golden.py records the
reference's outputs for, rebuilt identically by tests/test_oracle_vs_reference.py (CPU, fresh run of oracle/_ref) and by
tests/test_gpu_reference_parity.py (GPU, recorded outputs only)."""
import hashlib
import os

import numpy as np

from eagleeverything_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLDEN_CASES = ["geno_150x100", "genoDemo_150x4998", "synth_203x1531"]
SMOKE_CASE = "smoke_150x1000"
ALL_CASES = GOLDEN_CASES + [SMOKE_CASE]
NA = np.nan


def require_ref():
    """The reference builds, or the one permitted skip: a clone with neither the reference sources nor a built oracle/_ref."""
    import pytest
    from oracle import oracle_ref
    if oracle_ref.available():
        return oracle_ref
    if oracle_ref.sources_present():
        pytest.fail("oracle/_ref is not built although the reference sources are present: run build()")
    pytest.skip("neither the reference sources nor a built oracle/_ref exist here")


def case_inputs(case):
    """dict(M8 n x L int8, S, V, ahat, and for golden cases P, y, varG, X, varE, MMt).  SMOKE_CASE: __graft_entry__.smoke()'s seeds."""
    if case == SMOKE_CASE:
        n, L = 150, 1000
        Mt8 = synth.genotypes_marker_major(n, L, seed=1)
        rng = np.random.default_rng(0)
        A = rng.standard_normal((n, n)) / np.sqrt(n)
        S = A @ A.T + np.eye(n)
        V = 0.5 * np.eye(n) - 0.01 * np.outer(A[:, 0], A[:, 0])
        ahat = rng.standard_normal(n)
        y = rng.standard_normal(n)
        return {"M8": np.ascontiguousarray(Mt8.T), "S": S, "V": V, "ahat": ahat, "P": A @ A.T / n + np.eye(n), "y": y, "varG": 0.7}
    return dict(np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=False))


def masked_pair(L):
    """The two masked loci of the recorded scans: an inner one and the last."""
    return np.array([3.0, float(L - 1)])


def extract_loci(L):
    return [0, L // 2, L - 1]


def na_sets(n, seed=0):
    """test_reshape_host._na_sets (kept identical; asserted in test_oracle_vs_reference)."""
    rng = np.random.default_rng(seed)
    return {
        "empty": [],
        "first": [0],
        "last": [n - 1],
        "first_and_last": [n - 1, 0],
        "all_but_one": [i for i in range(n) if i != n // 2],
        "random_unsorted": list(rng.permutation(n)[: max(1, n // 10)]),
    }


def write_text_table(path, M8):
    """The 0/1/2 table the converters read: one line per individual, blanks between genotypes."""
    with open(path, "w") as f:
        for row in np.asarray(M8, dtype=np.int64) + 1:
            f.write(" ".join(map(str, row)) + "\n")
    return path


def file_digest(path):
    with open(path, "rb") as f:
        b = f.read()
    return "%s:%d" % (hashlib.sha256(b).hexdigest(), len(b))


def scrub(msgs, d):
    """message() lines with the scratch directory replaced, so that recorded texts compare across runs."""
    return [m.replace(str(d), "<DIR>") for m in msgs]


def error_inputs(d):
    """The error exits of test_ingest.test_gpu_ingest_errors_match_oracle, rebuilt from its seed: name -> (path, type, AA, AB, BB,
    dims).  Imports test_ingest's generators so that the inputs are the same by construction."""
    from test_ingest import _write, random_ped, random_text_table
    rng = np.random.default_rng(9)
    rows, _ = random_text_table(rng, 64, 40)
    out = {}
    bad = list(rows)
    bad[30] = bad[30].replace("BB", "Q", 1)
    bad[45] = " ".join(bad[45].split()[:-1])
    out["text_token"] = (_write(d / "b.txt", bad), "text", "AA", "AB", "BB", [64, 40])
    # test_ingest's own "unequal columns" input has a row with 41 tokens.  The reference stores token i into a vector of dims[1]
    # chars before it counts the columns (CreateASCIInospace.cpp:85-92 against :110), so a row that is too LONG is a heap overflow
    # there: undefined, not parity material.  The same exit is reached, defined, by a row that is too short.
    short = list(rows)
    short[7] = " ".join(short[7].split()[:-1])
    out["text_columns"] = (_write(d / "s.txt", short), "text", "AA", "AB", "BB", [64, 40])
    ped = random_ped(rng, 50, 30, p_missing=0.0)
    t = ped[33].split()
    t[6 + 2 * 17] = "Z"
    ped[33] = " ".join(t)
    t = ped[40].split()
    t[6] = "0"
    ped[40] = " ".join(t)
    out["plink_alleles"] = (_write(d / "q.ped", ped), "PLINK", "-9", "-9", "-9", [50, 66])
    ped[12] = ped[12] + " A"
    out["plink_columns"] = (_write(d / "c.ped", ped), "PLINK", "-9", "-9", "-9", [50, 66])
    return out
