"""What the int8 W engine keeps WITH S between calls, and its one pass per operand (csrc/eagle_w8.hip, csrc/eagle_host.h: w8_keep_valid).

S = MMt^-1/2 is the same matrix in every find_qtl call of an AM() run: its digit image, row statistics and the vectors S 1, S^T 1 are made
once and found in place by the calls that follow -- on the caller's declaration for a device-resident image (eagle_dev_declare_s;
DeviceShard.set_operands), on the verdict of the cached S for the reference-shaped call.  Nothing here is a tolerance: every number must
be bit for bit what a context that keeps nothing returns, whatever was kept, forgotten, re-declared or re-allocated in between; and the
fused row pass (statistics + digits from one read of the row) must write the bytes of the two kernels it replaces."""
import ctypes as C
import os

import numpy as np
import pytest

from eagleeverything_amd._lib import TUNE

pytestmark = pytest.mark.gpu

L_MARKERS = 1024
SHAPES = [(700, 768),     # n is not a multiple of 16; three tiles
          (1500, 1536),   # = W8_VBLOCK: one pipelined block
          (1600, 1792)]   # two pipelined blocks, the second one short
_OPERANDS = {}


def _api():
    from eagleeverything_amd import rcpp_api
    return rcpp_api


def _fresh(n):
    """A shard on a context nobody has used: every context of the process is closed first."""
    import torch
    from eagleeverything_amd.sharded import DeviceShard
    _api().close_all()
    sh = DeviceShard(n, L_MARKERS)
    if n in _OPERANDS:
        sh.Mt8.copy_(_OPERANDS[n]["Mt8"])
    sh.mode = 1
    sh.w_mode = 2
    return torch, sh


def _operands(n):
    """S, V, a_hat from the model algebra on a small synthetic panel (as tests/test_gpu_w8.py builds them), a second V and a second S;
    made once per size and left as they are."""
    if n not in _OPERANDS:
        from test_gpu_w8 import _model_operands
        torch, sh = _fresh(n)
        sh.fill_synthetic(seed=11)
        S, V, ahat = _model_operands(torch, sh)
        gen = torch.Generator(device=sh.dev)
        gen.manual_seed(3)
        g = torch.randn((n, 4), generator=gen, device=sh.dev, dtype=torch.float64)
        V2 = 1.25 * V + 1e-3 * float(V.diagonal().mean()) * (g @ g.T) / 4.0
        S2 = S + 1e-3 * float(S.diagonal().mean()) * torch.eye(n, dtype=torch.float64, device=sh.dev)
        _OPERANDS[n] = {"S": S, "V": V, "ahat": ahat, "V2": 0.5 * (V2 + V2.T), "S2": S2, "Mt8": sh.Mt8.clone()}
    return _OPERANDS[n]


def _image(torch, sh, Mx):
    out = torch.zeros((sh.np_, sh.np_), dtype=torch.float64, device=sh.dev)
    out[:sh.n, :sh.n] = Mx.t()
    return out


def _take(torch, sh):
    sh.scan()
    torch.cuda.synchronize()
    Lm = sh.Lloc
    return {"Wu": sh.Wu.clone(), "v": sh.v.clone(), "a": sh.a[:Lm].clone(), "vara": sh.vara[:Lm].clone(), "info": sh.w_info(),
            "best": sh.best()[:2]}


def _same(torch, x, y):
    for k in ("Wu", "v", "a", "vara"):
        assert torch.equal(x[k], y[k]), k
    assert x["info"] == y["info"], (x["info"], y["info"])
    assert x["best"] == y["best"], (x["best"], y["best"])


def _first_call(n, S, V, ahat):
    torch, sh = _fresh(n)
    sh.set_operands(S, V, ahat)
    r = _take(torch, sh)
    assert r["info"]["int8"] == 1, r["info"]
    return r


@pytest.mark.parametrize("n,n_pad", SHAPES)
def test_kept_s_returns_the_bits_of_a_context_that_keeps_nothing(n, n_pad):
    op = _operands(n)
    api = _api()
    first_v2 = _first_call(n, op["S"], op["V2"], op["ahat"])
    runs = {}
    for declare in (True, False):
        torch, sh = _fresh(n)
        assert sh.np_ == n_pad
        sh.declare_s = declare
        sh.set_operands(op["S"], op["V"], op["ahat"])
        c1 = _take(torch, sh)
        c2 = _take(torch, sh)
        sh.Va.copy_(_image(torch, sh, op["V2"]))        # another V, S as declared
        c3 = _take(torch, sh)
        runs[declare] = (c1, c2, c3)
        assert api.w8_keep_stats() == ((2, 1) if declare else (0, 3))
        assert c1["info"]["int8"] == 1, c1["info"]
    fresh = runs[True][0]                                # a fresh context's first call
    for declare in (True, False):
        _same(torch, runs[declare][0], fresh)
        _same(torch, runs[declare][1], fresh)
        _same(torch, runs[declare][2], first_v2)
    assert not torch.equal(first_v2["Wu"], fresh["Wu"])


@pytest.mark.parametrize("n,n_pad", SHAPES)
def test_a_new_s_a_released_image_and_a_grown_workspace_start_over(n, n_pad):
    from eagleeverything_amd.sharded import DeviceShard
    op = _operands(n)
    api = _api()
    first_s2 = _first_call(n, op["S2"], op["V"], op["ahat"])
    torch, sh = _fresh(n)
    sh.set_operands(op["S"], op["V"], op["ahat"])
    c1 = _take(torch, sh)
    assert not torch.equal(c1["Wu"], first_s2["Wu"])
    # another S in the same buffer, declared again
    sh.Sa.copy_(_image(torch, sh, op["S2"]))
    sh._check(sh.L.eagle_dev_declare_s(sh.ctx, sh.Sa.data_ptr(), sh.n, sh.np_))
    _same(torch, _take(torch, sh), first_s2)
    _same(torch, _take(torch, sh), first_s2)
    assert api.w8_keep_stats() == (1, 2)
    # released and set again
    sh.release_operands()
    sh.set_operands(op["S2"], op["V"], op["ahat"])
    _same(torch, _take(torch, sh), first_s2)
    _same(torch, _take(torch, sh), first_s2)
    assert api.w8_keep_stats() == (2, 3)
    # the workspace grows for a larger n_pad on the same context (that shard declares nothing: sh's declaration stands), then back
    big = DeviceShard(n + 300, 256)
    assert big.ctx == sh.ctx and big.np_ > sh.np_
    big.mode, big.w_mode, big.declare_s = 1, 2, False
    eye = torch.eye(big.n, dtype=torch.float64, device=big.dev)
    big.set_operands(0.9 * eye, 0.5 * eye, torch.ones(big.n, dtype=torch.float64, device=big.dev))
    big.scan_operands()
    torch.cuda.synchronize()
    _same(torch, _take(torch, sh), first_s2)
    _same(torch, _take(torch, sh), first_s2)
    h, m = api.w8_keep_stats()
    assert h == 3 and m == 5, (h, m)


def _probe(torch, sh, M, cuts, asym):
    np_ = sh.np_
    dev = sh.dev
    out = {"slices": torch.full((6, np_, np_), 99, dtype=torch.int8, device=dev), "vec3": torch.full((3, np_), -7.0, dtype=torch.float64, device=dev),
           "e": torch.full((np_,), -99, dtype=torch.int32, device=dev), "dssq": torch.full((6, np_), -1, dtype=torch.int64, device=dev),
           "stats": torch.zeros(128, dtype=torch.uint8, device=dev)}
    arr = (C.c_long * len(cuts))(*cuts)
    sh._check(sh.L.eagle_w8_probe_rows(sh.ctx, M.data_ptr(), np_, arr, len(cuts), int(asym), out["slices"].data_ptr(), out["vec3"].data_ptr(),
                                       out["e"].data_ptr(), out["dssq"].data_ptr(), out["stats"].data_ptr(), sh._stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n,n_pad", SHAPES)
def test_one_pass_over_a_row_writes_what_the_two_kernels_write(n, n_pad):
    op = _operands(n)
    torch, sh = _fresh(n)
    sh.set_operands(op["S"], op["V"], op["ahat"])
    sh.scan_operands()
    torch.cuda.synchronize()
    assert sh.w_info()["int8"] == 1
    X = sh.tmp.clone()                                   # X = S V^T, the second product's operand
    blocks = [[0, n_pad]] + ([[0, 1536, n_pad]] if n_pad > 1536 else []) + [[0, 1, 257, n_pad]]
    try:
        for M, asym in ((sh.Sa, 1), (sh.Va, 1), (X, 0)):
            for cuts in blocks:
                sh.L.eagle_dev_set_tune(sh.ctx, TUNE["W8_ROWPASS_SPLIT"])      # the two-kernel form
                two = _probe(torch, sh, M, cuts, asym)
                sh.L.eagle_dev_set_tune(sh.ctx, TUNE["SHIPPED"])
                one = _probe(torch, sh, M, cuts, asym)
                for k in two:
                    assert torch.equal(one[k], two[k]), (k, cuts, asym)
                assert int(two["e"].min()) > -99 and float(two["vec3"][1].max()) > 0.0 and int(two["slices"][0].abs().max()) > 0
    finally:
        sh.L.eagle_dev_set_tune(sh.ctx, TUNE["SHIPPED"])


@pytest.mark.parametrize("devices", [0, (0, 0)])
def test_reference_shaped_calls_keep_s_on_the_cache_verdict(tmp_path, monkeypatch, devices):
    """Three calculate_a_and_vara_rcpp calls, another V on the second, another S on the third: the bits of the same sequence with the
    cached S switched off (EAGLE_HIP_NO_SCACHE: every call uploads S, nobody vouches for it, nothing is kept)."""
    from eagleeverything_amd import synth
    api = _api()
    n, Lm = 700, L_MARKERS
    nd = len(devices) if isinstance(devices, tuple) else 1
    Mt8 = synth.genotypes_marker_major(n, Lm, seed=4)
    rng = np.random.default_rng(2)
    A = rng.standard_normal((n, 30)) / np.sqrt(n)
    S = np.eye(n) * 0.8 + A @ A.T
    S = 0.5 * (S + S.T)
    B = rng.standard_normal((n, n)) * 1e-3
    V = 0.5 * np.eye(n) - 0.05 * (A[:, :5] @ A[:, :5].T) + 0.5 * (B + B.T)
    V2 = 1.1 * V
    S2 = S + 1e-3 * np.eye(n)
    ahat = rng.standard_normal(n)
    geno = synth.write_geno_pair(str(tmp_path), Mt8)
    monkeypatch.setenv("EAGLE_HIP_W_MODE", "2")
    seqs = {}
    try:
        for no_cache in (False, True):
            if no_cache:
                monkeypatch.setenv("EAGLE_HIP_NO_SCACHE", "1")
            api.close_all()
            out = []
            for Sx, Vx in ((S, V), (S, V2), (S2, V)):
                r = api.calculate_a_and_vara_rcpp(geno["asciifileMt"], np.nan, Sx, Vx, 8.0, (Lm, n), ahat, device=devices)
                assert api.last_w_info(device=devices)["int8"] == 1
                out.append((r["a"].copy(), r["vara"].copy(), api.last_scan_argmax(device=devices)[:2]))
                if len(out) == 2:
                    mid = (api.scan_operand_cache_stats(device=devices), api.w8_keep_stats(device=devices))
            seqs[no_cache] = out
            cache, keep = api.scan_operand_cache_stats(device=devices), api.w8_keep_stats(device=devices)
            if no_cache:
                assert cache == (0, 0) and keep[0] == 0 and keep[1] == 3 * nd, (cache, keep)
            else:
                assert mid == ((nd, 0), (nd, nd)), mid          # the second call: S verified, its products found in place
                assert cache == (nd, nd), cache                 # the third: another S, every device starts over ...
                assert keep[1] >= 2 * nd, keep                  # ... and computes its products anew
        for x, y in zip(seqs[False], seqs[True]):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
        assert not np.array_equal(seqs[False][0][1], seqs[False][1][1]) and not np.array_equal(seqs[False][0][1], seqs[False][2][1])
    finally:
        monkeypatch.delenv("EAGLE_HIP_NO_SCACHE", raising=False)
        api.close_all()


def test_declined_operands_keep_nothing_and_the_next_good_s_works():
    n = 700
    op = _operands(n)
    api = _api()
    good = _first_call(n, op["S"], op["V"], op["ahat"])
    torch, sh = _fresh(n)
    Snan = op["S"].clone()
    Snan[3, 5] = float("nan")
    Snan[5, 3] = float("nan")
    gen = torch.Generator(device=sh.dev)
    gen.manual_seed(1)
    Sasym = op["S"] + 1e-7 * float(op["S"].diagonal().mean()) * torch.triu(torch.randn(op["S"].shape, generator=gen, device=sh.dev, dtype=torch.float64), 1)
    hits = 0
    for Sbad, why in ((Snan, 1), (Sasym, 2)):
        sh.set_operands(Sbad, op["V"], op["ahat"])
        for _ in range(2):                               # declined both times, and the second call finds nothing kept
            sh.w_mode = 2
            sh.scan_operands()
            torch.cuda.synchronize()
            info = sh.w_info()
            assert info["int8"] == 0 and info["declined"] == why, info
            W8 = sh.Wu.clone()
            sh.w_mode = 0                                # declined as before: the fp64 products' image
            sh.scan_operands()
            torch.cuda.synchronize()
            assert torch.equal(torch.isnan(W8), torch.isnan(sh.Wu))
            assert torch.equal(torch.nan_to_num(W8), torch.nan_to_num(sh.Wu))
        assert api.w8_keep_stats()[0] == hits
        sh.w_mode = 2
        sh.set_operands(op["S"], op["V"], op["ahat"])   # the next good S
        _same(torch, _take(torch, sh), good)
        _same(torch, _take(torch, sh), good)
        hits += 1
        assert api.w8_keep_stats()[0] == hits
