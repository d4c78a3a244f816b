"""ReshapeM_rcpp (E/src/ReshapeM_rcpp.cpp) in FILES mode, on the host: eagle_reshape_m(NULL, ..., EAGLE_RESHAPE_FILES) against the
reference's own ReshapeM_rcpp.cpp (oracle/_ref) and a Python restatement of its rewrite, the same writer (csrc/eagle_reshape.h) under ASan + UBSan, and the AM() driver on a
trait with NaN against the complete-case run.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_CASES, ROOT
from eagleeverything_amd import am, r_api, rcpp_api, synth
from eagleeverything_amd._lib import EagleError

from test_am_driver import OracleBackend, _planted


def reference_reshape(fM, fMt, indxNA):
    """ReshapeM_rcpp.cpp:17-120 restated: lines of M whose 0-based number is in indxNA dropped, the characters at indxNA erased
    from every line of Mt in decreasing order, every line written with '\\n'.  Returns (M bytes, Mt bytes, newdims)."""
    na = sorted(indxNA, reverse=True)
    with open(fM, "rb") as f:
        lines = f.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines = lines[:-1]
    kept = [ln for i, ln in enumerate(lines) if i not in set(na)]
    newdims = [len(kept), len(lines[-1]) if lines else 0]
    with open(fMt, "rb") as f:
        tl = f.read().split(b"\n")
    if tl and tl[-1] == b"":
        tl = tl[:-1]
    out_t = []
    for ln in tl:
        b = bytearray(ln)
        for i in na:
            del b[i]
        out_t.append(bytes(b))
    return b"".join(x + b"\n" for x in kept), b"".join(x + b"\n" for x in out_t), newdims


def _pair(tmp_path, name):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    geno = synth.write_geno_pair(str(tmp_path), np.ascontiguousarray(g["M8"].T))
    return geno


def _na_sets(n, seed=0):
    rng = np.random.default_rng(seed)
    return {
        "empty": [],
        "first": [0],
        "last": [n - 1],
        "first_and_last": [n - 1, 0],
        "all_but_one": [i for i in range(n) if i != n // 2],
        "random_unsorted": list(rng.permutation(n)[: max(1, n // 10)]),
    }


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_files_mode_matches_reference_bytes(tmp_path, case):
    from oracle import oracle_ref as ref   # the reference's own ReshapeM_rcpp.cpp on the stand-in headers (oracle/_ref)
    # where no reference checkout was ever built the restatement stands alone, as before; this test never skips
    assert ref.available() or not ref.sources_present(), "oracle/_ref is not built although the reference sources are present: run build()"
    geno = _pair(tmp_path, case)
    n, L = geno["dim_of_ascii_M"]
    for label, na in _na_sets(n).items():
        exp_m, exp_t, exp_dims = reference_reshape(geno["asciifileM"], geno["asciifileMt"], na)
        # the reference wants indxNA in decreasing order (ReshapeM_rcpp.cpp:103), this project takes any order
        if ref.available():
            assert ref.ReshapeM_rcpp(geno["asciifileM"], geno["asciifileMt"], sorted(na, reverse=True), (n, L)) == exp_dims, label
            with open(geno["asciifileM"] + "tmp", "rb") as f:
                assert f.read() == exp_m, label
            with open(geno["asciifileMt"] + "tmp", "rb") as f:
                assert f.read() == exp_t, label
            os.remove(geno["asciifileM"] + "tmp")
            os.remove(geno["asciifileMt"] + "tmp")
        dims = rcpp_api.ReshapeM_rcpp(geno["asciifileM"], geno["asciifileMt"], na, (n, L))
        assert dims == exp_dims == [n - len(na), L], label
        with open(geno["asciifileM"] + "tmp", "rb") as f:
            assert f.read() == exp_m, label
        with open(geno["asciifileMt"] + "tmp", "rb") as f:
            assert f.read() == exp_t, label


def test_files_mode_unterminated_and_uneven_lines(tmp_path):
    fM, fMt = str(tmp_path / "M.ascii"), str(tmp_path / "Mt.ascii")
    with open(fM, "wb") as f:
        f.write(b"0120\n22\n\n1112")  # uneven lines, an empty one, no final line end
    with open(fMt, "wb") as f:
        f.write(b"0201\n120112\n2101")
    for na in ([3, 1], [0], [2]):
        exp_m, exp_t, exp_dims = reference_reshape(fM, fMt, na)
        assert r_api.ReshapeM(fM, fMt, np.asarray(na) + 1, (4, 4)) == exp_dims
        assert open(fM + "tmp", "rb").read() == exp_m
        assert open(fMt + "tmp", "rb").read() == exp_t


def test_files_mode_errors(tmp_path):
    geno = _pair(tmp_path, "geno_150x100")
    fM, fMt, dims = geno["asciifileM"], geno["asciifileMt"], geno["dim_of_ascii_M"]
    L = rcpp_api._lib.load()
    for na, code in (([3, 3], -3), ([150], -3), ([-1], -3)):
        with pytest.raises(EagleError) as e:
            rcpp_api.ReshapeM_rcpp(fM, fMt, na, dims)
        assert e.value.code == code
        assert L.eagle_last_error(None).decode() == e.value.text
    with pytest.raises(EagleError) as e:
        rcpp_api.ReshapeM_rcpp(str(tmp_path / "missing"), fMt, [1], dims)
    assert e.value.code == -1 and "Could not open" in e.value.text
    with pytest.raises(EagleError) as e:
        rcpp_api.ReshapeM_rcpp(fM, str(tmp_path / "missing"), [1], dims)
    assert e.value.code == -1
    short = str(tmp_path / "short")
    with open(short, "w") as f:
        f.write("012\n")
    with pytest.raises(EagleError) as e:  # a line of Mt that does not reach the largest index
        rcpp_api.ReshapeM_rcpp(fM, short, [5], dims)
    assert e.value.code == -2


def test_check_for_na_in_trait():
    assert r_api.check_for_NA_in_trait(np.array([1.0, 2.0])).size == 0
    np.testing.assert_array_equal(r_api.check_for_NA_in_trait(np.array([np.nan, 1.0, np.nan, 3.0, np.nan])), [5, 3, 1])


DRIVER = r"""
#include "eagle_reshape.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
    // argv: M Mt n threads idx...
    std::vector<long> idx;
    for (int i = 5; i < argc; i++) idx.push_back(atol(argv[i]));
    std::vector<long> na;
    if (const char* why = reshape_check_na(idx.data(), (long)idx.size(), atol(argv[3]), na)) { printf("ARG %s\n", why); return 0; }
    std::vector<int32_t> keep = reshape_keep_list(atol(argv[3]), na);
    long nd[2];
    std::string msg;
    int rc = reshape_write_files(argv[1], argv[2], na, atoi(argv[4]), nd, msg);
    printf("rc=%d newdims=%ld,%ld keep=%zu %s\n", rc, nd[0], nd[1], keep.size(), msg.c_str());
    return 0;
}
"""


def test_writer_under_asan_ubsan(tmp_path):
    src = tmp_path / "reshape_driver.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "reshape_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "eagleeverything_amd", "csrc"), str(src), "-o", exe])
    geno = _pair(tmp_path, "synth_203x1531")
    n = geno["dim_of_ascii_M"][0]
    for na, threads in (([], 1), ([0, 202, 17], 4), ([i for i in range(n) if i != 5], 3), ([4, 4], 2), ([203], 2)):
        r = subprocess.run([exe, geno["asciifileM"], geno["asciifileMt"], str(n), str(threads)] + [str(i) for i in na],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        if len(set(na)) != len(na) or any(i >= n for i in na):
            assert r.stdout.startswith("ARG"), r.stdout
            continue
        exp_m, exp_t, exp_dims = reference_reshape(geno["asciifileM"], geno["asciifileMt"], na)
        assert "rc=0 newdims=%d,%d keep=%d" % (exp_dims[0], exp_dims[1], n - len(na)) in r.stdout, r.stdout
        assert open(geno["asciifileM"] + "tmp", "rb").read() == exp_m
        assert open(geno["asciifileMt"] + "tmp", "rb").read() == exp_t


def test_am_with_nan_trait_equals_complete_case(oracle, tmp_path):
    """AM.R:320-370: rows whose trait or covariate is NA are dropped from trait, X and both genotype files.  The driver on the
    NaN trait (FILES mode through the default reshape) must equal the driver on the complete-case trait and X with files
    rewritten by the restatement above."""
    geno, y, X, _ = _planted(tmp_path)
    n = y.size
    rng = np.random.default_rng(11)
    X = np.column_stack([X, rng.standard_normal(n)])
    y_na, X_na = y.copy(), X.copy()
    drop_trait = rng.choice(n, 9, replace=False)
    y_na[drop_trait] = np.nan
    drop_x = np.setdiff1d(rng.choice(n, 4, replace=False), drop_trait)
    X_na[drop_x, 1] = np.nan
    dropped = np.union1d(drop_trait, drop_x)
    keep = np.setdiff1d(np.arange(n), dropped)

    d2 = tmp_path / "cc"
    d2.mkdir()
    exp_m, exp_t, exp_dims = reference_reshape(geno["asciifileM"], geno["asciifileMt"], list(dropped))
    (d2 / "M.ascii").write_bytes(exp_m)
    (d2 / "Mt.ascii").write_bytes(exp_t)
    geno_cc = {"asciifileM": str(d2 / "M.ascii"), "asciifileMt": str(d2 / "Mt.ascii"), "dim_of_ascii_M": tuple(exp_dims)}
    ref = am.AM(y[keep], X[keep], geno_cc, maxit=6, backend=OracleBackend(oracle))
    res = am.AM(y_na, X_na, geno, maxit=6, backend=OracleBackend(oracle))
    assert res["all_picks"] == ref["all_picks"] and res["selected_loci"] == ref["selected_loci"]
    assert res["extBIC_trace"] == ref["extBIC_trace"]
    np.testing.assert_array_equal(res["indxNA"], np.sort(dropped + 1)[::-1])
    assert res["dim_of_ascii_M"] == exp_dims
    assert len(ref["all_picks"]) >= 2
    # a complete trait: no reshape, no *tmp files
    os.remove(geno["asciifileM"] + "tmp")
    full = am.AM(y, X, geno, maxit=3, backend=OracleBackend(oracle))
    assert full["indxNA"].size == 0 and not os.path.exists(geno["asciifileM"] + "tmp")
