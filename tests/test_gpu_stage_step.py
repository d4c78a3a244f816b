"""The tile engine's stage step (csrc/eagle_t8.h: X_DF, XRead, tx_kstep1_s .. tx_klast_s) in k_vara_i8p: the DMA sequences and the
fragment-read addresses advance inside the asm of the k-steps instead of in C++ between them.  No stage moves, no MFMA changes its
operands or its place, so every integer sum is the one of the form before it, which stays behind EAGLE_HIP_STAGE_GLUE=1 (csrc/eagle_ctx.h; read
at every launch, like the library's other test hooks -- the kernel-form switch keeps its closed list of names): the int64 q block, a
and vara are compared by equality, between the two forms and against the integer truth of tests/exact_scan.py.

What can go wrong is the bookkeeping where a sequence starts: the step to the other LDS buffer, the source step inside a tile, and the
one step per operand and tile that crosses into the next tile (another K stage, another column tile's descriptor; the empty descriptor
behind the last tile).  The shapes walk those: n = 300 (n_pad 512: two column tiles, a pad of 212 >= 128, so the last K stage of W is
dead), 500 (pad 12, nothing dropped), 700 (n_pad 768: three column tiles = a pair and a middle tile); L = 385 markers (one 384-row tile
and a ragged one) and 3 * 384 * 8 + 1 (more than one round of workers per XCD with a cut last round); 1 and 3 digit slices; and one case
under the paced instantiation.  W is handed over ready-made (DeviceShard.set_W)."""
import contextlib
import functools
import os

import numpy as np
import pytest

import exact_scan as ex
from eagleeverything_amd._lib import TUNE

pytestmark = pytest.mark.gpu
SHIPPED, PACED, UNPIPED = TUNE["SHIPPED"], TUNE["VARA_PACED"], TUNE["W8_UNPIPED"]
GLUE = "glue"     # not a switch value: the shipped switch value with EAGLE_HIP_STAGE_GLUE=1 in the environment
POISON = 0xA5
L_SHORT, L_ROUNDS = 385, 3 * 384 * 8 + 1
SCAN_SHAPES = [(n, L) for n in (300, 500, 700) for L in (L_SHORT, L_ROUNDS)]


@functools.lru_cache(maxsize=None)
def _case(n, L, S):
    """S = 3: the dense case of exact_scan at u = 1 (three digits hold W).  S = 1: |x| <= 3, one digit holds the folded entries."""
    case = ex.build_case(n, L, log2u=0, small=(S == 1))
    ex.check_exact(case)
    a, vara, _ = ex.scan_truth(case)
    return case, a, vara


def _tune(sh, v):
    sh.L.eagle_dev_set_tune(sh.ctx, int(v))


@contextlib.contextmanager
def _form(sh, form):
    """The switch value `form`, or for GLUE the shipped value under the environment hook; both undone on the way out."""
    _tune(sh, SHIPPED if form == GLUE else form)
    if form == GLUE:
        os.environ["EAGLE_HIP_STAGE_GLUE"] = "1"
    try:
        yield
    finally:
        os.environ.pop("EAGLE_HIP_STAGE_GLUE", None)
        _tune(sh, SHIPPED)


def _kernel(torch, sh, tune, smax):
    """prepare on a poisoned workspace + the vara kernel under `tune` -> (q block of all smax slots, vara, a, S used, e)."""
    with _form(sh, tune):
        sh._ws().fill_(POISON)
        sh.vara_prepare()
        sh.vara_kernel()
        torch.cuda.synchronize()
    S_used = sh.vara_i8_info()[0]
    q = sh.ws[256:256 + 8 * smax * sh.Lp].view(torch.int64).clone()
    return q, sh.vara[:sh.Lloc].clone(), sh.a[:sh.Lloc].clone(), S_used, sh.last_e


def _scan(n, L, S, tunes):
    import torch
    from eagleeverything_amd.sharded import DeviceShard
    case, a, vara = _case(n, L, S)
    sh = DeviceShard(n, L)
    sh.Mt8[:L, :n] = torch.from_numpy(case["Mt8"].copy()).to(sh.dev)
    sh.mode, sh.nslices = 1, S
    try:
        sh.set_W(np.ldexp(case["X"].astype(np.float64), case["log2u"]), case["ahat"])
        sh.scan_operands()
        out = {t: _kernel(torch, sh, t, S) for t in tunes}
    finally:
        _tune(sh, SHIPPED)
    what = "n=%d L=%d S=%d" % (n, L, S)
    q0, v0, a0, S_used, e = out[tunes[0]]
    print(what, "n_pad", sh.np_, "S used", S_used, "e", e)
    assert S_used == S and int(q0.abs().max()) > 0, what
    for t in tunes[1:]:
        assert torch.equal(out[t][0], q0), "q differs: %s, form %s against %s" % (what, t, tunes[0])
        assert torch.equal(out[t][1], v0), "vara differs: %s, form %s against %s" % (what, t, tunes[0])
        assert torch.equal(out[t][2], a0), "a differs: %s, form %s against %s" % (what, t, tunes[0])
    # the truth applies where the S digits hold W exactly: the unit of the last digit at or below the step 2 u of the folded entries
    assert 2.0 ** (e + 2 - 8 * S_used) <= 2.0 * 2.0 ** case["log2u"], (what, e, S_used)
    np.testing.assert_array_equal(a0.cpu().numpy(), a, err_msg=what)
    bad = np.flatnonzero(v0.cpu().numpy() != vara)
    assert bad.size == 0, "%s: vara of %d markers, first %d: %r, truth %r" % (what, bad.size, bad[0], float(v0[bad[0]]), vara[bad[0]])


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("n,L", SCAN_SHAPES)
def test_scan_step_is_the_glue_form_and_the_integer_truth(n, L, S):
    _scan(n, L, S, (SHIPPED, GLUE))


def test_scan_step_under_the_paced_instantiation():
    """k_vara_i8p<true> (soft barrier per column-tile pair) has the step too: three column tiles, several rounds, against both unpaced forms."""
    _scan(700, L_ROUNDS, 3, (PACED, SHIPPED, GLUE))


# ---- k_w8_gemm_p: a digit pair is to the step what a column tile is to the scan kernel ----
# n = 1,300 and 1,500 (n_pad 1,536: four 384-column tiles; the individuals end inside the last one) and 1,537 (n_pad 1,792: five, the
# last one 256 rows short -- its descriptor covers the rows there are, at every pair change too); the operands of tests/exact_w8.py,
# whose plane pairs lie inside every configuration: the rule picks the smallest, (3, 4), whose level
# groups hold one pair (level 2: the step's pair change never runs, the empty descriptor follows the first pair), two and three pairs
# (levels 3 and 4: one and two pair changes per workgroup) -- several groups, several pairs per group.  The library has no smaller
# configuration and no way to force one, so a (1, 2) configuration cannot be run; its one-pair group is level 2 of (3, 4).
W8_CASES = [(1300, "s1"), (1300, "s2"), (1500, "s1"), (1500, "s2"), (1537, "s2")]


@functools.lru_cache(maxsize=None)
def _w8_case(n, kind):
    import exact_w8 as xw
    case = xw.build_case(n, kind)
    truth = xw.check_exact(case)
    return case, truth


@pytest.mark.parametrize("n,kind", W8_CASES)
def test_w_engine_step_is_the_glue_form_the_unpiped_engine_and_the_integer_truth(n, kind):
    import torch
    import exact_w8 as xw
    from eagleeverything_amd.sharded import DeviceShard
    case, truth = _w8_case(n, kind)
    sh = DeviceShard(n, 129)
    sh.set_operands(case["S"][:n, :n].copy(), case["V"][:n, :n].copy(), case["ahat"][:n].copy())
    sh.mode, sh.w_mode = 1, 2
    sh.L.eagle_dev_set_spectral(sh.ctx, 0)
    out = {}
    try:
        for t in (SHIPPED, GLUE, UNPIPED):
            with _form(sh, t):
                sh.tmp.fill_(float("nan"))
                sh.Wu.fill_(float("nan"))
                sh.scan_operands()
                torch.cuda.synchronize()
            info = sh.w_info()
            what = "n=%d %s form %s" % (n, kind, t)
            assert info["int8"] == 1 and info["declined"] == 0, (what, info)
            assert xw.covered(truth["pairs1"], info["k1"], info["T1"]) and xw.covered(truth["pairs2"], info["k2"], info["T2"]), (what, info)
            out[t] = (sh.tmp.cpu().numpy().copy(), sh.Wu.cpu().numpy().copy(), (info["k1"], info["T1"], info["k2"], info["T2"]))
    finally:
        _tune(sh, SHIPPED)
        sh.L.eagle_dev_set_spectral(sh.ctx, 1)
    X0, W0, cfg = out[SHIPPED]
    print("n=%d %s n_pad %d configurations (k, T): product 1 (%d, %d), product 2 (%d, %d)" % ((n, kind, sh.np_) + cfg))
    assert sh.np_ == (1792 if n == 1537 else 1536) and cfg[1] >= 4 and cfg[3] >= 4           # at least levels 2..4: groups of one, two and three pairs
    for t in (GLUE, UNPIPED):
        assert out[t][2] == cfg
        assert np.array_equal(out[t][0], X0), "X = S V^T differs: n=%d %s form %s" % (n, kind, t)
        assert np.array_equal(out[t][1], W0), "folded W differs: n=%d %s form %s" % (n, kind, t)
    assert np.array_equal(X0, truth["tmp"]), "X = S V^T against the integer truth"
    assert np.array_equal(W0, truth["Wu"]), "folded W against the integer truth"
