"""eagle_reshape_m VIEW aliases on the MI355X: every entry point that reads a genotype file must give, on the view, exactly what
it gives on the files FILES mode (= the reference's ReshapeM_rcpp) rewrote -- bit for bit -- on every load path: text, the 2-bit
sidecar, sidecars disabled, a resident source (k_gather_cols_i8), streamed windows, a two-sub-context eagle_open_devices
context.  Plus the padding boundaries, staleness, and AM() on a trait with NaN."""
import os
import shutil

import numpy as np
import pytest

from eagleeverything_amd import am, rcpp_api, synth
from eagleeverything_amd._lib import EagleError

from test_am_driver import OracleBackend

pytestmark = pytest.mark.gpu
NA = np.nan


def _pairs(tmp_path, Mt8, na):
    """The same source pair in two directories: FILES mode rewrites the one, VIEW mode registers aliases on the other."""
    df, dv = tmp_path / "files", tmp_path / "view"
    df.mkdir(exist_ok=True)
    dv.mkdir(exist_ok=True)
    gf = synth.write_geno_pair(str(df), Mt8)
    gv = {"asciifileM": str(dv / "M.ascii"), "asciifileMt": str(dv / "Mt.ascii"), "dim_of_ascii_M": gf["dim_of_ascii_M"]}
    shutil.copyfile(gf["asciifileM"], gv["asciifileM"])
    shutil.copyfile(gf["asciifileMt"], gv["asciifileMt"])
    return gf, gv


def _reshape_both(gf, gv, na, device=0):
    dims = gf["dim_of_ascii_M"]
    nd_f = rcpp_api.ReshapeM_rcpp(gf["asciifileM"], gf["asciifileMt"], na, dims)
    nd_v = rcpp_api.ReshapeM_rcpp(gv["asciifileM"], gv["asciifileMt"], na, dims, view=True, device=device)
    assert nd_f == nd_v
    mk = lambda g: {"asciifileM": g["asciifileM"] + "tmp", "asciifileMt": g["asciifileMt"] + "tmp", "dim_of_ascii_M": tuple(nd_f)}
    assert not os.path.exists(gv["asciifileM"] + "tmp") and not os.path.exists(gv["asciifileMt"] + "tmp")
    return mk(gf), mk(gv)


def _operands(n, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    S = A @ A.T + np.eye(n)
    V = 0.5 * np.eye(n) - 0.01 * np.outer(A[:, 0], A[:, 0])
    return S, V, rng.standard_normal(n), rng.standard_normal(n), A @ A.T / n + np.eye(n)


def _all_calls(g, device):
    n, L = g["dim_of_ascii_M"]
    S, V, ahat, y, P = _operands(n)
    out = {}
    out["mmt"] = rcpp_api.calculateMMt_rcpp(g["asciifileM"], 8.0, 2, NA, (n, L), device=device)
    res = rcpp_api.calculate_a_and_vara_rcpp(g["asciifileMt"], NA, S, V, 8.0, (L, n), ahat, device=device)
    out["a"], out["vara"] = res["a"], res["vara"]
    out["argmax"] = rcpp_api.last_scan_argmax(device=device)[:2]
    out["ar"] = rcpp_api.calculate_reduced_a_rcpp(g["asciifileMt"], 0.7, P, y, 8.0, (n, L), NA, device=device)
    out["geno"] = [rcpp_api.extract_geno_rcpp(g["asciifileM"], 8.0, c, (n, L), device=device) for c in (0, L // 2, L - 1)]
    out["rb"] = [rcpp_api.ReadBlock(g["asciifileMt"], r0, n, k, device=device) for r0, k in ((0, 3), (L - 5, 5))]
    out["rbM"] = rcpp_api.ReadBlock(g["asciifileM"], n - 2, L, 2, device=device)
    out["rc"] = [rcpp_api.getRowColumn(g["asciifileM"], device=device), rcpp_api.getRowColumn(g["asciifileMt"], device=device)]
    return out


def _assert_equal(x, y):
    assert x.keys() == y.keys()
    for k in x:
        a, b = x[k], y[k]
        if isinstance(a, list):
            assert len(a) == len(b), k
            for u, v in zip(a, b):
                assert np.array_equal(np.asarray(u), np.asarray(v)), k
        else:
            assert np.array_equal(np.asarray(a), np.asarray(b)), k


def _check(tmp_path, Mt8, na, device=0, prime=None, paths=None):
    """VIEW calls equal FILES calls bit for bit; `paths` = {source: expected number of windows or None for "some"} of the view's
    loads (rcpp_api.view_load_counts), the sources not named must not have been used."""
    gf, gv = _pairs(tmp_path, Mt8, na)
    if prime:
        prime(gv)
    ff, vv = _reshape_both(gf, gv, na, device=device)
    before = rcpp_api.view_load_counts(device)
    view = _all_calls(vv, device)
    after = rcpp_api.view_load_counts(device)
    files = _all_calls(ff, device)
    _assert_equal(view, files)
    used = {k: after[k] - before[k] for k in after}
    for k, v in used.items():
        if paths is None:
            continue
        if k in paths:
            assert v > 0 if paths[k] is None else v == paths[k], (k, used)
        else:
            assert v == 0, (k, used)
    return ff, vv, view


def _demo_Mt8(golden):
    return np.ascontiguousarray(golden("genoDemo_150x4998")["M8"].T)


NA_DEMO = [149, 0, 77, 3, 4, 5, 120, 64, 63, 10, 11, 98, 31, 140, 141]


def test_view_bit_equal_text_and_oracle(golden, oracle, tmp_path):
    ff, vv, view = _check(tmp_path, _demo_Mt8(golden), NA_DEMO, paths={"text": None})
    n, L = vv["dim_of_ascii_M"]
    assert (n, L) == (150 - len(NA_DEMO), 4998)
    assert np.array_equal(view["mmt"], oracle.calculateMMt_rcpp(ff["asciifileM"], 8.0, 2, NA, (n, L)))
    S, V, ahat, _, _ = _operands(n)
    exp = oracle.calculate_a_and_vara_rcpp(ff["asciifileMt"], NA, S, V, 8.0, (L, n), ahat)
    np.testing.assert_allclose(view["vara"], exp["vara"], rtol=1e-7)
    with np.errstate(all="ignore"):
        tsq, tsq_ref = view["a"] ** 2 / view["vara"], exp["a"] ** 2 / exp["vara"]
    ok = np.isfinite(tsq_ref) & (tsq_ref > 0)
    assert np.max(np.abs(tsq[ok] - tsq_ref[ok]) / tsq_ref[ok]) <= 1e-6
    assert view["argmax"][0] == oracle.tsq_argmax(exp["a"], exp["vara"])[1]


def test_view_from_sidecar(golden, tmp_path):
    """Mt.ascii (and its .e2b) made by the converter from M.ascii, then dropped from HBM: the view reads the sidecar
    (k_unpack2b_cols)."""
    Mt8 = _demo_Mt8(golden)

    def prime(g):
        n, L = g["dim_of_ascii_M"]
        os.remove(g["asciifileMt"])
        rcpp_api.createMt_ASCII_rcpp(g["asciifileM"], g["asciifileMt"], "text", 8.0, (n, L))
        assert os.path.exists(g["asciifileMt"] + ".e2b")
        rcpp_api.drop_cache()

    _check(tmp_path, Mt8, NA_DEMO, prime=prime, paths={"sidecar": None, "text": None})   # Mt: the sidecar; M: text


def test_view_sidecar_disabled(golden, tmp_path, monkeypatch):
    monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")
    rcpp_api.drop_cache()
    Mt8 = _demo_Mt8(golden)

    def prime(g):  # a sidecar is there, and must not be read
        n, L = g["dim_of_ascii_M"]
        os.remove(g["asciifileMt"])
        monkeypatch.setenv("EAGLE_HIP_SIDECAR", "1")
        rcpp_api.createMt_ASCII_rcpp(g["asciifileM"], g["asciifileMt"], "text", 8.0, (n, L))
        monkeypatch.setenv("EAGLE_HIP_SIDECAR", "0")
        assert os.path.exists(g["asciifileMt"] + ".e2b")
        rcpp_api.drop_cache()

    _check(tmp_path, Mt8, NA_DEMO, prime=prime, paths={"text": None})


def test_view_from_resident_source(golden, tmp_path):
    """A call on the source files first leaves their images resident: the Mt view is one k_gather_cols_i8, the M view row copies."""
    def prime(g):
        n, L = g["dim_of_ascii_M"]
        S, V, ahat, _, _ = _operands(n)
        rcpp_api.calculateMMt_rcpp(g["asciifileM"], 8.0, 2, NA, (n, L))
        rcpp_api.calculate_a_and_vara_rcpp(g["asciifileMt"], NA, S, V, 8.0, (L, n), ahat)

    rcpp_api.drop_cache()
    _check(tmp_path, _demo_Mt8(golden), NA_DEMO, prime=prime, paths={"resident": None})


def test_view_streamed(golden, tmp_path, monkeypatch):
    monkeypatch.setenv("EAGLE_HIP_MAX_RESIDENT_GB", "0.0006")
    rcpp_api.drop_cache()
    _check(tmp_path, _demo_Mt8(golden), NA_DEMO, paths={"text": None})
    assert rcpp_api.last_stream_stats()["chunks"] > 1


def test_view_two_subcontexts(golden, tmp_path):
    _check(tmp_path, _demo_Mt8(golden), NA_DEMO, device=(0, 0), paths={"text": None})


@pytest.mark.parametrize("n,na", [(257, [0, 256]), (513, [300])])
def test_view_padding_boundaries(tmp_path, n, na):
    Mt8 = synth.genotypes_marker_major(n, 700, seed=n)
    _check(tmp_path, Mt8, na, paths={"text": None})


def test_identity_view(golden, tmp_path):
    _check(tmp_path, _demo_Mt8(golden)[:1000], [])


def test_non_fixed_width_source_uses_line_scanner(golden, tmp_path):
    """A source with CRLF line ends in places is not fixed-width: the general scanner serves both views, as it would read the
    rewritten files."""
    Mt8 = _demo_Mt8(golden)[:700]
    gf, gv = _pairs(tmp_path, Mt8, NA_DEMO)
    for g in (gf, gv):
        for f in (g["asciifileM"], g["asciifileMt"]):
            lines = open(f, "rb").read().split(b"\n")
            lines[1] = lines[1] + b"\r"
            open(f, "wb").write(b"\n".join(lines))
    ff, vv = _reshape_both(gf, gv, NA_DEMO)
    before = rcpp_api.view_load_counts()
    n, L = vv["dim_of_ascii_M"]
    for g in (vv, ff):
        g["mmt"] = rcpp_api.calculateMMt_rcpp(g["asciifileM"], 8.0, 2, NA, (n, L))
        g["rb"] = rcpp_api.ReadBlock(g["asciifileMt"], 0, n, L)
    assert np.array_equal(vv["mmt"], ff["mmt"]) and np.array_equal(vv["rb"], ff["rb"])
    assert rcpp_api.view_load_counts()["scanner"] - before["scanner"] >= 2


def test_files_mode_replaces_a_view(golden, tmp_path):
    """VIEW with one NA set, then FILES with another of the same size on the same names: the context must read the new files."""
    Mt8 = _demo_Mt8(golden)[:900]
    _, gv = _pairs(tmp_path, Mt8, NA_DEMO)
    dims = gv["dim_of_ascii_M"]
    rcpp_api.ReshapeM_rcpp(gv["asciifileM"], gv["asciifileMt"], NA_DEMO, dims, view=True)
    tM, tMt = gv["asciifileM"] + "tmp", gv["asciifileMt"] + "tmp"
    n, L = 150 - len(NA_DEMO), 900
    old = rcpp_api.calculateMMt_rcpp(tM, 8.0, 2, NA, (n, L))              # the view's image is resident now
    na_b = [(i + 1) % 150 for i in NA_DEMO]   # another set of the same size
    assert rcpp_api.ReshapeM_rcpp(gv["asciifileM"], gv["asciifileMt"], na_b, dims) == [n, L]
    assert not rcpp_api.is_view(tM) and os.path.exists(tM)
    cM, cMt = str(tmp_path / "copyM.ascii"), str(tmp_path / "copyMt.ascii")
    shutil.copyfile(tM, cM)
    shutil.copyfile(tMt, cMt)
    new = rcpp_api.calculateMMt_rcpp(tM, 8.0, 2, NA, (n, L))
    assert np.array_equal(new, rcpp_api.calculateMMt_rcpp(cM, 8.0, 2, NA, (n, L)))
    assert not np.array_equal(new, old)
    assert np.array_equal(rcpp_api.ReadBlock(tMt, 0, n, L), rcpp_api.ReadBlock(cMt, 0, n, L))
    assert rcpp_api.getRowColumn(tMt) == rcpp_api.getRowColumn(cMt)


def test_view_of_changed_source_fails(golden, tmp_path):
    Mt8 = _demo_Mt8(golden)[:600]
    gf, gv = _pairs(tmp_path, Mt8, NA_DEMO)
    ff, vv = _reshape_both(gf, gv, NA_DEMO)
    n, L = vv["dim_of_ascii_M"]
    first = rcpp_api.calculateMMt_rcpp(vv["asciifileM"], 8.0, 2, NA, (n, L))   # resident now
    Mt8b = Mt8.copy()
    Mt8b[:, 7] = -Mt8b[:, 7]
    synth.write_ascii(gv["asciifileMt"], Mt8b)
    synth.write_ascii(gv["asciifileM"], np.ascontiguousarray(Mt8b.T))
    for f in (gv["asciifileM"], gv["asciifileMt"]):
        st = os.stat(f)
        os.utime(f, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    S, V, ahat, _, _ = _operands(n)
    with pytest.raises(EagleError) as e:
        rcpp_api.calculateMMt_rcpp(vv["asciifileM"], 8.0, 2, NA, (n, L))
    assert e.value.code == -2
    with pytest.raises(EagleError) as e:
        rcpp_api.calculate_a_and_vara_rcpp(vv["asciifileMt"], NA, S, V, 8.0, (L, n), ahat)
    assert e.value.code == -2
    with pytest.raises(EagleError):
        rcpp_api.extract_geno_rcpp(vv["asciifileM"], 8.0, 0, (n, L))
    # registering again serves the new bits
    rcpp_api.ReshapeM_rcpp(gv["asciifileM"], gv["asciifileMt"], NA_DEMO, (150, 600), view=True)
    again = rcpp_api.calculateMMt_rcpp(vv["asciifileM"], 8.0, 2, NA, (n, L))
    assert again.shape == first.shape


def test_am_with_nan_trait_view_vs_files_vs_oracle(golden, oracle, tmp_path):
    g = golden("genoDemo_150x4998")
    rng = np.random.default_rng(5)
    y = g["y"].astype(np.float64).copy()
    y[rng.choice(y.size, 15, replace=False)] = np.nan
    gf, gv = _pairs(tmp_path, np.ascontiguousarray(g["M8"].T), [])
    view = am.AM(y, g["X"], gv, maxit=6)                                  # HipBackend: VIEW mode
    assert not os.path.exists(gv["asciifileM"] + "tmp")
    files = am.AM(y, g["X"], gf, maxit=6, backend=_FilesHip())            # the HIP loop on rewritten files
    ref = am.AM(y, g["X"], gf, maxit=6, backend=OracleBackend(oracle))    # the oracle loop on rewritten files
    assert view["indxNA"].size == 15 and view["dim_of_ascii_M"] == [135, 4998]
    assert view["all_picks"] == files["all_picks"] == ref["all_picks"]
    assert view["selected_loci"] == ref["selected_loci"]
    np.testing.assert_allclose(view["extBIC_trace"], ref["extBIC_trace"], rtol=1e-9)
    assert view["extBIC_trace"] == files["extBIC_trace"]
    assert len(view["all_picks"]) >= 2


class _FilesHip(am.HipBackend):
    def reshape(self, geno, indxNA):
        return am.reshape_geno(geno, indxNA, view=False)
