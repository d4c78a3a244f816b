"""CPU: the C oracle (oracle/eagle_oracle*.c) against the reference's OWN src/*.cpp, compiled unmodified on the functional
stand-in headers of oracle/refstub (oracle/_ref/libeagle_ref.so, and libeagle_ref_ld.so with long-double accumulation).  What
this pins is the reference's control flow, index arithmetic, file parsing, branch rules and texts; the inner dot products are
the stand-in's (order i, j, k).

fp64 gate (a, vara, reduced a): the expected value is the long-double build; the reference's own fp64 build lies at distance
d = max|x64 - xld| / max|xld| from it; the oracle passes within 4 d (another, equally valid summation order), capped at the 1e-10
that DESIGN section 9 claims.  d is measured here from the two reference builds alone.  Integer and byte outputs are exact.

Inputs where the reference itself is undefined are not parity material; DESIGN section 9 lists each with its line.  These tests
skip only where neither the reference sources nor a built oracle/_ref exist; with sources and no build they fail ("run build()").
"""
import json
import os

import numpy as np
import pytest

import refpin
from refpin import GOLDEN_CASES, NA
from eagleeverything_amd import synth

CAP = 1e-10


@pytest.fixture(scope="module")
def ref():
    return refpin.require_ref()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    out = {}
    for case in GOLDEN_CASES:
        g = refpin.case_inputs(case)
        d = tmp_path_factory.mktemp(case)
        out[case] = (g, synth.write_geno_pair(str(d), np.ascontiguousarray(g["M8"].T)), d)
    return out


def dist(x, xld):
    return float(np.max(np.abs(np.ravel(x) - np.ravel(xld))) / np.max(np.abs(xld)))


def gate_check(name, x_oracle, x64, xld):
    d_ref = dist(x64, xld)
    d_or = dist(x_oracle, xld)
    gate = min(4.0 * d_ref, CAP)
    print("%s: reference fp64 to long double %.3e, oracle to long double %.3e, gate %.3e" % (name, d_ref, d_or, gate))
    assert d_or <= gate, (name, d_or, gate)
    return d_ref


# ---------------------------------------------------------------------------------------------------------------- ReadBlock
@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_readblock(case, files, ref, oracle):
    g, geno, _ = files[case]
    n, L = g["M8"].shape
    windows = [("asciifileM", 0, L, n), ("asciifileMt", 0, n, L),                  # whole files
               ("asciifileM", 0, L, 1), ("asciifileM", n - 1, L, 1),              # first row, last row
               ("asciifileMt", 7, n - 5, 11), ("asciifileMt", L - 3, n, 3), ("asciifileM", 5, 1, n - 5), ("asciifileMt", L - 1, 1, 1)]
    for key, start, cols, rows in windows:
        a, b = oracle.ReadBlock(geno[key], start, cols, rows), ref.ReadBlock(geno[key], start, cols, rows)
        assert a.shape == b.shape == (rows, cols)
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ref.ReadBlock(geno["asciifileM"], 0, L, n), g["M8"].astype(np.float64))
    with pytest.raises(ref.OracleError) as e:
        ref.ReadBlock(geno["asciifileM"] + ".absent", 0, 3, 3)
    assert e.value.code == -1 and e.value.text == "ERROR: Could not open  %s\n" % (geno["asciifileM"] + ".absent")
    with pytest.raises(oracle.OracleError, match="Could not open"):
        oracle.ReadBlock(geno["asciifileM"] + ".absent", 0, 3, 3)


# ------------------------------------------------------------------------------------------------------- calculateMMt_rcpp
def mmt_mem_for_rows(r, L):
    """max_memory_in_Gbytes that makes calculateMMt_rcpp.cpp:103-106 give r rows per block: the middle of the interval of budgets
    for which floor((-2L + sqrt(4L^2 + 4 mem 1e9 / 8)) / 2.2) == r."""
    return ((2.2 * (r + 0.5) + 2.0 * L) ** 2 - 4.0 * L * L) / 5e8


# rows per block chosen per case: one that divides n and one that does not; the resulting block counts are stated
MMT_BLOCKS = {"geno_150x100": ((50, 3), (40, 4)), "genoDemo_150x4998": ((50, 3), (40, 4)), "synth_203x1531": ((29, 7), (40, 6))}


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_mmt(case, files, ref, oracle):
    g, geno, _ = files[case]
    n, L = g["M8"].shape
    fM = geno["asciifileM"]
    sels = {"NA": NA, "one": np.array([5.0]), "several": np.array([3.0, 17.0, 64.0]), "first_and_last": np.array([0.0, float(L - 1)]),
            "NA_first": np.array([NA, 3.0, 17.0])}
    for label, sel in sels.items():
        m_ref, rows_ref = ref.calculateMMt_rcpp(fM, 8.0, 2, sel, (n, L), return_branch=True)
        m_or, rows_or = oracle.calculateMMt_rcpp(fM, 8.0, 2, sel, (n, L), return_branch=True)
        assert rows_ref == rows_or == 0, label                                           # the in-memory branch
        np.testing.assert_array_equal(m_or, m_ref, err_msg=label)
        for rows, nblocks in MMT_BLOCKS[case]:
            mem = mmt_mem_for_rows(rows, L)
            assert mem < (n * n * 8 + 2 * n * L * 8) / 1e9
            b_ref, rows_ref = ref.calculateMMt_rcpp(fM, mem, 2, sel, (n, L), return_branch=True)
            b_or, rows_or = oracle.calculateMMt_rcpp(fM, mem, 2, sel, (n, L), return_branch=True)
            assert rows_ref == rows_or == rows and -(-n // rows) == nblocks and (n % rows == 0) == (rows in (50, 29)), (label, rows)
            np.testing.assert_array_equal(b_ref, m_ref, err_msg=label)
            np.testing.assert_array_equal(b_or, b_ref, err_msg=label)
    np.testing.assert_array_equal(ref.calculateMMt_rcpp(fM, 8.0, 2, NA, (n, L)), g["MMt"].astype(np.float64))
    assert ref.messages() == [" Number of cores being used for calculation is .. 2"]


# ----------------------------------------------------------------------------------------------- calculate_a_and_vara_rcpp
@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_scan_in_memory(case, files, ref, oracle):
    g, geno, _ = files[case]
    n, L = g["M8"].shape
    fMt = geno["asciifileMt"]
    rng = np.random.default_rng(5)
    V_ns = g["V"] + 0.05 * np.abs(g["V"]).max() * rng.standard_normal((n, n))            # a non-symmetric dim_reduced_vara
    assert not np.allclose(V_ns, V_ns.T)
    for label, sel, V in (("NA", NA, g["V"]), ("masked", g["sel_masked"], g["V"]), ("first_last", np.array([0.0, float(L - 1)]), g["V"]),
                          ("nonsym", NA, V_ns), ("nonsym_masked", np.array([7.0]), V_ns)):
        args = (fMt, sel, g["S"], V, 8.0, (L, n), g["ahat"])
        r64, nb = ref.calculate_a_and_vara_rcpp(*args, return_branch=True)
        rld = ref.calculate_a_and_vara_rcpp(*args, ld=True)
        ror, br = oracle.calculate_a_and_vara_rcpp(*args, return_branch=True)
        assert nb == 0 and br == 0
        for k in ("a", "vara"):
            assert ror[k].shape == r64[k].shape == (L, 1)
            gate_check("%s %s %s" % (case, label, k), ror[k], r64[k], rld[k])
            np.testing.assert_array_equal(ror[k] == 0.0, rld[k] == 0.0)                  # the same rows masked
        if not np.isnan(np.ravel(sel)[0]):
            for s in np.ravel(sel).astype(int):
                assert rld["a"][s, 0] == 0.0 and rld["vara"][s, 0] == 0.0
        assert oracle.tsq_argmax(ror["a"], ror["vara"])[1] == oracle.tsq_argmax(rld["a"], rld["vara"])[1]


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_scan_memory_test_is_an_integer_division(case, files, ref, oracle):
    """calculate_a_and_vara_rcpp.cpp:65 divides integers: 4 L n 8 / 1e9 is 0 for every golden case, so any positive budget takes
    the in-memory branch.  Real division would give 4.8e-4 .. 2.4e-2 and send a budget of 1e-5 to the block branch."""
    g, geno, _ = files[case]
    n, L = g["M8"].shape
    mem = 1e-5
    assert 0 < mem < 4.0 * n * L * 8 / 1e9 and (4 * n * L * 8) // 1000000000 == 0
    args = (geno["asciifileMt"], NA, g["S"], g["V"], mem, (L, n), g["ahat"])
    r64, nblocks = ref.calculate_a_and_vara_rcpp(*args, return_branch=True)
    assert nblocks == 0 and not any("Increasing maxmemGb" in m for m in ref.messages())
    ror, br = oracle.calculate_a_and_vara_rcpp(*args, return_branch=True)
    assert br == 0
    rld = ref.calculate_a_and_vara_rcpp(*args, ld=True)
    for k in ("a", "vara"):
        gate_check("%s %s" % (case, k), ror[k], r64[k], rld[k])
    assert oracle.tsq_argmax(ror["a"], ror["vara"])[1] == oracle.tsq_argmax(rld["a"], rld["vara"])[1]
    # the sentinel of :133-144 (negative budget) with its texts
    neg = ref.calculate_a_and_vara_rcpp(geno["asciifileMt"], NA, g["S"], g["V"], -1.0, (L, n), g["ahat"])
    assert neg["a"].shape == (1,) and neg["a"][0] == 0 and neg["vara"][0] == 0
    assert ref.messages() == [" Increasing maxmemGb would improve performance... \n", "\n", "Error:  availmemGb is set to -1",
                              "        Cannot even read in a single row of data into memory.",
                              "        Please increase availmemGb for this data set.", "\n", " multiple_locus_am has terminated with errors\n"]
    neg_or = oracle.calculate_a_and_vara_rcpp(geno["asciifileMt"], NA, g["S"], g["V"], -1.0, (L, n), g["ahat"])
    assert neg_or["a"].shape == (1,) and neg_or["a"][0] == 0 and neg_or["vara"][0] == 0


def test_scan_block_branch_and_its_bounds(ref, oracle, tmp_path):
    """The marker-block branch (:117-234) needs 4 L n 8 >= 1e9: n = 48, L = 700000.  availmemGb = 0.5 gives
    0.5e9 / (4 * 48 * 8) = 325520 rows per block, 3 blocks; block 1 starts at marker 325520.  Masked: the last marker of block 0,
    the first of block 1 (the boundary itself), the one after, the first and last marker of the file."""
    n, L = 48, 700000
    rng = np.random.default_rng(1)
    Mt8 = rng.integers(-1, 2, size=(L, n), dtype=np.int8)
    p = synth.write_ascii(str(tmp_path / "Mt.ascii"), Mt8)
    A = rng.standard_normal((n, n)) / 6.0
    S = A @ A.T + np.eye(n)
    V = 0.3 * np.eye(n) + 0.02 * rng.standard_normal((n, n))                             # non-symmetric
    ah = rng.standard_normal(n)
    rows = int(0.5 * 1000000000 / (4 * n * 8))
    assert rows == 325520 and (4 * n * L * 8) // 1000000000 == 1
    for label, sel in (("NA", NA), ("bounds", np.array([rows - 1.0, float(rows), rows + 1.0, 0.0, float(L - 1)]))):
        r64, nb = ref.calculate_a_and_vara_rcpp(p, sel, S, V, 0.5, (L, n), ah, return_branch=True)
        assert nb == 3 and ref.messages()[0] == " Increasing maxmemGb would improve performance... \n"
        assert ref.messages()[1:4:1][0] == "Performing block iteration ... 0"
        rld = ref.calculate_a_and_vara_rcpp(p, sel, S, V, 0.5, (L, n), ah, ld=True)
        ror, br = oracle.calculate_a_and_vara_rcpp(p, sel, S, V, 0.5, (L, n), ah, return_branch=True)
        assert br == rows and -(-L // br) == nb
        for k in ("a", "vara"):
            gate_check("blocked %s %s" % (label, k), ror[k], r64[k], rld[k])
            np.testing.assert_array_equal(ror[k] == 0.0, rld[k] == 0.0)
        assert oracle.tsq_argmax(ror["a"], ror["vara"])[1] == oracle.tsq_argmax(rld["a"], rld["vara"])[1], label
        if label == "bounds":
            z = np.flatnonzero(rld["vara"].ravel() == 0.0)
            np.testing.assert_array_equal(z, np.sort(sel.astype(int)))
            # the in-memory branch of the reference (availmemGb = 8 > 1) masks the same rows and gives the same numbers
            full, nb0 = ref.calculate_a_and_vara_rcpp(p, sel, S, V, 8.0, (L, n), ah, return_branch=True)
            assert nb0 == 0
            np.testing.assert_array_equal(full["a"], r64["a"])
            np.testing.assert_array_equal(full["vara"], r64["vara"])


# ------------------------------------------------------------------------------------------------ calculate_reduced_a_rcpp
@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_reduced_a(case, files, ref, oracle):
    """:56 multiplies by the integer sizeof(double) / 1e9 == 0: the in-memory branch runs for every budget > 0; for a budget <= 0
    the block branch computes a negative row count and returns its 1 x 1 null matrix (:92-103).  Those are its two reachable ends."""
    g, geno, _ = files[case]
    n, L = g["M8"].shape
    for label, sel, mem in (("NA", NA, 8.0), ("masked", np.array([5.0, 9.0, float(L - 1)]), 8.0), ("tiny", NA, 1e-12)):
        args = (geno["asciifileMt"], float(g["varG"]), g["P"], g["y"], mem, (n, L), sel)
        a64, ald, aor = ref.calculate_reduced_a_rcpp(*args), ref.calculate_reduced_a_rcpp(*args, ld=True), oracle.calculate_reduced_a_rcpp(*args)
        assert a64.shape == aor.shape == (L, 1)
        gate_check("%s reduced a %s" % (case, label), aor, a64, ald)
        np.testing.assert_array_equal(aor == 0.0, ald == 0.0)
    for mem in (0.0, -2.0):
        args = (geno["asciifileMt"], float(g["varG"]), g["P"], g["y"], mem, (n, L), NA)
        z_ref, z_or = ref.calculate_reduced_a_rcpp(*args), oracle.calculate_reduced_a_rcpp(*args)
        assert z_ref.shape == z_or.shape == (1, 1) and z_ref[0, 0] == z_or[0, 0] == 0.0
        assert ref.messages()[0] == " Note:  Increasing availmemGb would improve performance... " and ref.messages()[-1] == "AM has terminated with errors\n"


# ------------------------------------------------------------------------------------------------------- extract_geno_rcpp
@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_extract_geno(case, files, ref, oracle):
    g, geno, _ = files[case]
    n, L = g["M8"].shape
    blocked = 7.5 * 8 * L / 1e9          # :53 -> 7 rows per block, 22 or 29 blocks, the last one short
    assert int(blocked * 1e9 / (8 * L)) == 7 and blocked < n * L * 8 / 1e9
    for c in (0, L // 2, L - 1):
        for mem in (8.0, blocked):
            got = ref.extract_geno_rcpp(geno["asciifileM"], mem, c, (n, L))
            np.testing.assert_array_equal(got, oracle.extract_geno_rcpp(geno["asciifileM"], mem, c, (n, L)))
            np.testing.assert_array_equal(got, g["M8"][:, c].astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------- converters
def _same(a, b):
    with open(a, "rb") as f, open(b, "rb") as h:
        return f.read() == h.read()


def test_getRowColumn(ref, oracle, tmp_path):
    for name in ("geno_150x100.txt", "geno_150x100.ped"):
        p = os.path.join(refpin.GOLDEN, name)
        assert ref.getRowColumn(p) == oracle.getRowColumn(p)
    assert ref.getRowColumn(os.path.join(refpin.GOLDEN, "geno_150x100.ped")) == [150, 206]
    q = tmp_path / "t.txt"
    q.write_text("a b  c\nd e f\nlast line without newline")
    assert ref.getRowColumn(str(q)) == oracle.getRowColumn(str(q)) == [3, 3]
    with pytest.raises(ref.OracleError) as e:
        ref.getRowColumn(str(tmp_path / "absent"))
    assert e.value.text == "\n\n ERROR: Could not open  %s\n\n\n" % (tmp_path / "absent")
    with pytest.raises(oracle.OracleError):
        oracle.getRowColumn(str(tmp_path / "absent"))


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_converters_text(case, files, ref, oracle):
    g, geno, d = files[case]
    n, L = g["M8"].shape
    txt = refpin.write_text_table(str(d / "table.txt"), g["M8"])
    ok_r, msgs = ref.createM_ASCII_rcpp(txt, str(d / "rM"), "text", 0, 1, 2, 8, [n, L])
    ok_o, info = oracle.createM_ASCII_rcpp(txt, str(d / "oM"), "text", 0, 1, 2, 8, [n, L])
    assert ok_r and ok_o and info["kind"] == "ok"
    assert _same(d / "rM", d / "oM") and _same(d / "rM", geno["asciifileM"])
    assert msgs[0] == " First 5 lines and 12 columns of the marker text  file. " and len(msgs) == 6
    for mem in (8.0, 3.5 * n * 3 * 11.5 / 1e9):     # whole file; column blocks of 11 (createMt_ASCII_rcpp.cpp:133), the last one short
        ref.createMt_ASCII_rcpp(str(d / "rM"), str(d / "rMt"), "text", mem, [n, L])
        oracle.createMt_ASCII_rcpp(str(d / "oM"), str(d / "oMt"), "text", mem, [n, L])
        assert _same(d / "rMt", d / "oMt") and _same(d / "rMt", geno["asciifileMt"])
    assert ref.messages()[-1] == " The marker file has been Uploaded"


def test_converters_plink_and_error_exits(ref, oracle, tmp_path):
    ped, gtxt = os.path.join(refpin.GOLDEN, "geno_150x100.ped"), os.path.join(refpin.GOLDEN, "geno_150x100.txt")
    for src, typ, codes, dims in ((ped, "PLINK", ("-9", "-9", "-9"), [150, 206]), (gtxt, "text", (0, 1, 2), [150, 100])):
        ok_r, _ = ref.createM_ASCII_rcpp(src, str(tmp_path / "rM"), typ, *codes, 8, dims)
        ok_o, _ = oracle.createM_ASCII_rcpp(src, str(tmp_path / "oM"), typ, *codes, 8, dims)
        assert ok_r and ok_o and _same(tmp_path / "rM", tmp_path / "oM")
        if typ == "PLINK":   # createMt_ASCII_rcpp with type PLINK: the bytes, and the type's way into the summary (:230-238)
            for mem in (8.0, 3.5 * 150 * 3 * 11.5 / 1e9):
                ref.createMt_ASCII_rcpp(str(tmp_path / "rM"), str(tmp_path / "rMt"), "PLINK", mem, [150, 100])
                oracle.createMt_ASCII_rcpp(str(tmp_path / "oM"), str(tmp_path / "oMt"), "PLINK", mem, [150, 100])
                assert _same(tmp_path / "rMt", tmp_path / "oMt")
                assert ref.messages()[-8:-4] == [" File type:                   PLINK", " Reformatted ASCII file name:  %s" % (tmp_path / "rM"),
                                                 " Number of individuals:        150", " Number of loci:               100"]
            lines = open(tmp_path / "rM").read().split("\n")[:-1]
            assert open(tmp_path / "rMt").read() == "".join("".join(ln[j] for ln in lines) + "\n" for j in range(100))
    # the two routines createM_ASCII_rcpp hands over to, called directly: the same files and texts as through it
    ok, direct = ref.CreateASCIInospace_PLINK(ped, str(tmp_path / "dM"), [150, 206])
    ok2, through = ref.createM_ASCII_rcpp(ped, str(tmp_path / "rM"), "PLINK", "-9", "-9", "-9", 8, [150, 206])
    assert ok and ok2 and direct == through and _same(tmp_path / "dM", tmp_path / "rM")
    ok, direct = ref.CreateASCIInospace(gtxt, str(tmp_path / "dM"), [150, 100], 0, 1, 2, quiet=False)
    ok2, through = ref.createM_ASCII_rcpp(gtxt, str(tmp_path / "rM"), "text", 0, 1, 2, 8, [150, 100], quiet=False)
    assert ok and ok2 and through == [" A text file is being assumed as the input data file type. "] + direct and _same(tmp_path / "dM", tmp_path / "rM")
    # hand-built PLINK rows: missing alleles first, late second allele, '-' and '0'
    from test_ingest import _write, random_ped
    rows = random_ped(np.random.default_rng(4), 40, 25, p_missing=0.08)
    src = _write(tmp_path / "m.ped", rows)
    ok_r, msgs = ref.createM_ASCII_rcpp(src, str(tmp_path / "rM"), "PLINK", "-9", "-9", "-9", 8, [40, 56])
    ok_o, info = oracle.createM_ASCII_rcpp(src, str(tmp_path / "oM"), "PLINK", "-9", "-9", "-9", 8, [40, 56])
    assert ok_r and ok_o and _same(tmp_path / "rM", tmp_path / "oM")
    assert info["missing_seen"] == any("missing alleles" in m for m in msgs) is True
    # the error exits: what the oracle reports, written out as the reference words it
    for name, (src, typ, AA, AB, BB, dims) in refpin.error_inputs(tmp_path).items():
        ok_r, msgs = ref.createM_ASCII_rcpp(src, str(tmp_path / "rE"), typ, AA, AB, BB, 8, dims)
        ok_o, info = oracle.createM_ASCII_rcpp(src, str(tmp_path / "oE"), typ, AA, AB, BB, 8, dims)
        assert not ok_r and not ok_o, name
        assert _same(tmp_path / "rE", tmp_path / "oE"), name                             # the rows written before the failure
        if info["kind"] == "token":
            exp = ["\n Marker file contains marker genotypes that are different to AA=%s AB=%s BB=%s" % (AA, AB, BB),
                   " For example , %s in row %d" % (info["token"], info["row"]), "\n ReadMarker has terminated with errors\n"]
        elif info["kind"] == "columns":
            exp = ["\n", "Error:  %s contains an unequal number of columns per row.  " % ("PLINK file" if typ == "PLINK" else "Marker text file"),
                   "        The error has occurred at row %d which contains %d but " % (info["row"], info["columns"]),
                   "        it should contain %d columns of data. " % dims[1], "\n", " ReadMarkerData has terminated with errors"]
        else:
            assert info["kind"] == "alleles" and not info["missing_seen"]
            exp = ["\n", "Error:  PLINK file cannot contain more than two alleles at a locus.",
                   "        The error has occurred at snp locus %d for individual %d" % (info["locus"], info["row"]), "\n",
                   " ReadMarkerData has terminated with errors"]
        assert msgs == exp, name
    ok_r, msgs = ref.createM_ASCII_rcpp(str(tmp_path / "absent"), str(tmp_path / "rE"), "text", 0, 1, 2, 8, [3, 3])
    ok_o, info = oracle.createM_ASCII_rcpp(str(tmp_path / "absent"), str(tmp_path / "oE"), "text", 0, 1, 2, 8, [3, 3])
    assert not ok_r and not ok_o and info["kind"] == "open"
    assert msgs == ["ERROR: Text file could not be opened with filename  %s\n" % (tmp_path / "absent")]


# ------------------------------------------------------------------------------------------------------------- ReshapeM_rcpp
@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_reshape(case, files, ref):
    """The reference against this project's host writer (FILES mode opens no device) and against test_reshape_host's Python
    restatement, byte for byte.  The reference is given indxNA in decreasing order, its stated precondition
    (ReshapeM_rcpp.cpp:103; AM.R builds it so); this project accepts any order."""
    from eagleeverything_amd import rcpp_api
    from test_reshape_host import _na_sets, reference_reshape
    g, geno, d = files[case]
    n, L = g["M8"].shape
    fM, fMt = geno["asciifileM"], geno["asciifileMt"]
    assert {k: list(map(int, v)) for k, v in _na_sets(n).items()} == {k: list(map(int, v)) for k, v in refpin.na_sets(n).items()}
    for label, na in refpin.na_sets(n).items():
        nd = ref.ReshapeM_rcpp(fM, fMt, sorted(na, reverse=True), (n, L))
        got = [open(f + "tmp", "rb").read() for f in (fM, fMt)]
        exp_m, exp_t, exp_dims = reference_reshape(fM, fMt, na)
        assert nd == exp_dims == [n - len(na), L] and got == [exp_m, exp_t], label
        assert rcpp_api.ReshapeM_rcpp(fM, fMt, na, (n, L)) == nd, label
        assert [open(f + "tmp", "rb").read() for f in (fM, fMt)] == got, label


def test_reshape_order_is_kept_different_on_purpose(ref, tmp_path):
    """given indxNA in INCREASING order the reference erases character indxNA[k] of a line that has already lost
    k characters (ReshapeM_rcpp.cpp:104-106) -- the wrong individuals, or an index past the end of the line.  This project sorts."""
    from eagleeverything_amd import rcpp_api
    fM, fMt = str(tmp_path / "M.ascii"), str(tmp_path / "Mt.ascii")
    with open(fM, "w") as f:
        f.write("0000\n1111\n2222\n0120\n")
    with open(fMt, "w") as f:
        f.write("0120\n0121\n0122\n0120\n")
    assert ref.ReshapeM_rcpp(fM, fMt, [0, 1], (4, 4)) == [2, 4]
    assert open(fMt + "tmp").read() == "10\n11\n12\n10\n"          # characters 0 and 2 went, not 0 and 1
    assert ref.ReshapeM_rcpp(fM, fMt, [0, 3], (4, 4)) == [2, 4]
    assert open(fMt + "tmp").read() == "120\n121\n122\n120\n"     # index 3 of a line of 3 erases nothing: individual 3 stays
    with pytest.raises(ref.OracleError) as e:                       # index 3 of a line of 2: std::out_of_range in the reference
        ref.ReshapeM_rcpp(fM, fMt, [1, 2, 3], (4, 4))
    assert e.value.code == -2
    assert rcpp_api.ReshapeM_rcpp(fM, fMt, [0, 1], (4, 4)) == [2, 4]
    assert open(fMt + "tmp").read() == "20\n21\n22\n20\n" and open(fM + "tmp").read() == "2222\n0120\n"
    assert rcpp_api.ReshapeM_rcpp(fM, fMt, [0, 3], (4, 4)) == [2, 4]
    assert open(fMt + "tmp").read() == "12\n12\n12\n12\n"


# -------------------------------------------------------------------------------------------------- the committed recordings
@pytest.mark.parametrize("case", refpin.ALL_CASES)
def test_recorded_outputs_match_a_fresh_run(case, ref, tmp_path):
    """tests/golden/ref_<case>.npz against oracle/_ref now.  Integers, digests and texts exactly; fp64 values within the
    fp64-to-long-double distance of the same output (another compiler or libm may round a product differently)."""
    import sys
    sys.path.insert(0, refpin.GOLDEN)
    import make_ref_golden
    rec = dict(np.load(os.path.join(refpin.GOLDEN, "ref_%s.npz" % case), allow_pickle=False))
    fresh = make_ref_golden.record(case, tmp_path)
    assert set(rec) == set(fresh)
    for k in sorted(rec):
        if k.endswith("_json"):
            assert json.loads(str(rec[k])) == json.loads(str(fresh[k])), k
        elif k.endswith("_f64") or k.endswith("_ld"):
            base = k.rsplit("_", 1)[0]
            d = dist(rec[base + "_f64"], rec[base + "_ld"])
            assert d > 0 and dist(fresh[k], rec[k]) <= d, k
        else:
            assert rec[k].dtype == fresh[k].dtype
            np.testing.assert_array_equal(rec[k], fresh[k], err_msg=k)
