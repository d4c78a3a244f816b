#!/usr/bin/env python3
"""Generate tests/golden/ref_<case>.npz: what the reference's own src/*.cpp, built on the stand-in headers of oracle/refstub
(oracle/_ref, made by build() where the reference checkout exists), WROTE for the golden cases and for smoke()'s operands.
Recorded outputs only -- numbers, digests of written files and message texts; no program text.

Per case: MMt with and without masking (both branches agree, asserted here); a and vara from the fp64 build and from the
long-double build (rounded to fp64), for selected_loci NA and for two masked loci; reduced a; three extracted loci; ReadBlock
windows; SHA-256:length of every converter and reshape output file (createMt for type text and PLINK); the message() and stop
texts, those of the MM^T row-block branch (quiet and not) and of the scan's and reduced a's sentinel exits included.
tests/test_oracle_vs_reference.py::test_recorded_outputs_match_a_fresh_run keeps these files honest.
"""
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import refpin  # noqa: E402
from eagleeverything_amd import synth  # noqa: E402
from oracle import oracle_ref  # noqa: E402

NA = np.nan


def mmt_blocked_mem(n, L):
    need = (n * n * 8 + 2 * n * L * 8) / 1e9
    return need / 6.0


def record(case, d, ld_too=True):
    """-> dict of arrays (strings and lists as JSON text) for one case, from a fresh run of oracle/_ref in directory d.
    ld_too=False (the sanitizer run, which has one library only) fills the long-double entries from the fp64 build."""
    g = refpin.case_inputs(case)
    M8 = g["M8"]
    n, L = M8.shape
    geno = synth.write_geno_pair(str(d), np.ascontiguousarray(M8.T))
    fM, fMt = geno["asciifileM"], geno["asciifileMt"]
    sel = refpin.masked_pair(L)
    out, texts, digests = {}, {}, {}

    out["MMt"] = oracle_ref.calculateMMt_rcpp(fM, 8.0, 2, NA, (n, L)).astype(np.int32)
    out["MMt_masked"] = oracle_ref.calculateMMt_rcpp(fM, 8.0, 2, sel, (n, L)).astype(np.int32)
    texts["mmt_messages"] = oracle_ref.messages()
    for s, key in ((NA, "MMt"), (sel, "MMt_masked")):
        blk, rows = oracle_ref.calculateMMt_rcpp(fM, mmt_blocked_mem(n, L), 2, s, (n, L), return_branch=True)
        assert rows > 0 and np.array_equal(blk, out[key]), (case, key)
        assert np.array_equal(oracle_ref.calculateMMt_rcpp(fM, 8.0, 2, s, (n, L), ld=ld_too), out[key])
    for quiet, tag in ((True, "quiet"), (False, "loud")):   # the row-block branch says its block size whatever `quiet` is
        oracle_ref.calculateMMt_rcpp(fM, mmt_blocked_mem(n, L), 2, NA, (n, L), quiet=quiet)
        texts["mmt_block_messages_" + tag] = oracle_ref.messages()
    neg = oracle_ref.calculate_a_and_vara_rcpp(fMt, NA, g["S"], g["V"], -1.0, (L, n), g["ahat"])   # the sentinel of :133-144
    out["scan_sentinel"] = np.array([neg["a"], neg["vara"]])
    texts["scan_sentinel_messages"] = oracle_ref.messages()
    for s, tag in ((NA, "na"), (sel, "masked")):
        for ld, b in ((False, "f64"), (True, "ld")):
            r = oracle_ref.calculate_a_and_vara_rcpp(fMt, s, g["S"], g["V"], 8.0, (L, n), g["ahat"], ld=ld and ld_too)
            out["a_%s_%s" % (tag, b)], out["vara_%s_%s" % (tag, b)] = r["a"].ravel(), r["vara"].ravel()
    out["sel_masked"] = sel
    for ld, b in ((False, "f64"), (True, "ld")):
        out["ar_" + b] = oracle_ref.calculate_reduced_a_rcpp(fMt, float(g["varG"]), g["P"], g["y"], 8.0, (n, L), NA, ld=ld and ld_too).ravel()
    z = oracle_ref.calculate_reduced_a_rcpp(fMt, float(g["varG"]), g["P"], g["y"], 0.0, (n, L), NA)
    out["ar_sentinel"] = z
    texts["ar_sentinel_messages"] = oracle_ref.messages()
    out["extract_loci"] = np.array(refpin.extract_loci(L))
    out["extract"] = np.stack([oracle_ref.extract_geno_rcpp(fM, 8.0, c, (n, L)) for c in refpin.extract_loci(L)])
    out["readblock_Mt_7"] = oracle_ref.ReadBlock(fMt, 7, n - 5, 11).astype(np.int8)
    out["readblock_M_last"] = oracle_ref.ReadBlock(fM, n - 1, L, 1).astype(np.int8)

    # converters: the 0/1/2 table of the case -> M.ascii -> Mt.ascii
    txt = refpin.write_text_table(str(d / "table.txt"), M8)
    assert oracle_ref.getRowColumn(txt) == [n, L]
    ok, msgs = oracle_ref.createM_ASCII_rcpp(txt, str(d / "cM.ascii"), "text", 0, 1, 2, 8, [n, L])
    assert ok
    texts["createM_text_messages"] = refpin.scrub(msgs, d)
    digests["createM_text"] = refpin.file_digest(d / "cM.ascii")
    assert digests["createM_text"] == refpin.file_digest(fM)
    oracle_ref.createMt_ASCII_rcpp(str(d / "cM.ascii"), str(d / "cMt.ascii"), "text", 8, [n, L])
    texts["createMt_messages"] = refpin.scrub(oracle_ref.messages(), d)
    digests["createMt"] = refpin.file_digest(d / "cMt.ascii")
    assert digests["createMt"] == refpin.file_digest(fMt)
    for label, na in refpin.na_sets(n).items():
        # ReshapeM_rcpp.cpp:103 requires indxNA in decreasing order (AM.R passes it so); any other order is not parity material
        nd = oracle_ref.ReshapeM_rcpp(fM, fMt, sorted(na, reverse=True), (n, L))
        assert nd == [n - len(na), L]
        digests["reshape_%s_M" % label] = refpin.file_digest(fM + "tmp")
        digests["reshape_%s_Mt" % label] = refpin.file_digest(fMt + "tmp")

    if case == "geno_150x100":  # the reference's own data pair and the error exits
        ped, gtxt = os.path.join(HERE, "geno_150x100.ped"), os.path.join(HERE, "geno_150x100.txt")
        out["getRowColumn_ped"] = np.array(oracle_ref.getRowColumn(ped))
        out["getRowColumn_txt"] = np.array(oracle_ref.getRowColumn(gtxt))
        ok, msgs = oracle_ref.createM_ASCII_rcpp(ped, str(d / "pM.ascii"), "PLINK", "-9", "-9", "-9", 8, [150, 206])
        assert ok
        texts["createM_plink_messages"] = msgs
        digests["createM_plink"] = refpin.file_digest(d / "pM.ascii")
        oracle_ref.createMt_ASCII_rcpp(str(d / "pM.ascii"), str(d / "pMt.ascii"), "PLINK", 8, [150, 100])
        texts["createMt_plink_messages"] = refpin.scrub(oracle_ref.messages(), d)
        digests["createMt_plink"] = refpin.file_digest(d / "pMt.ascii")
        ok, msgs = oracle_ref.createM_ASCII_rcpp(gtxt, str(d / "tM.ascii"), "text", 0, 1, 2, 8, [150, 100])
        assert ok
        digests["createM_goldentxt"] = refpin.file_digest(d / "tM.ascii")
        for name, (src, typ, AA, AB, BB, dims) in refpin.error_inputs(d).items():
            ok, msgs = oracle_ref.createM_ASCII_rcpp(src, str(d / (name + ".ascii")), typ, AA, AB, BB, 8, dims)
            assert not ok
            texts["error_%s_messages" % name] = refpin.scrub(msgs, d)
            digests["error_" + name] = refpin.file_digest(d / (name + ".ascii"))
        for fn, args in (("ReadBlock", (str(d / "absent"), 0, 3, 3)), ("getRowColumn", (str(d / "absent"),))):
            try:
                getattr(oracle_ref, fn)(*args)
                raise AssertionError("no stop")
            except oracle_ref.OracleError as e:
                assert e.code == -1
                texts["stop_" + fn] = e.text.replace(str(d), "<DIR>")
    out["texts_json"] = np.array(json.dumps(texts, sort_keys=True))
    out["digests_json"] = np.array(json.dumps(digests, sort_keys=True))
    return out


def main():
    assert oracle_ref.available(), "run build() on a machine with the reference checkout first"
    for case in refpin.ALL_CASES:
        with tempfile.TemporaryDirectory() as d:
            out = record(case, Path(d))
        path = os.path.join(HERE, "ref_%s.npz" % case)
        np.savez_compressed(path, **out)
        print(case, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
