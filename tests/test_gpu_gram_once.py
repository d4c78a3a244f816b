"""The Gram product of the last-digit image is formed once (csrc/eagle_i8mfma.hip: k_gram_rowabs_i8<true>, k_gram_hi_settle).

Level 1 of the spectral bound needs the row sums of |Ds Ds|, level 2 needs E_hi = round(offdiag(Ds Ds) / 2^s), the sum of squares of what
the rounding leaves, the largest diagonal entry and an overflow flag: the same exact int32 product.  The level-1 kernel now leaves all of
it on the way; the two-kernel form (k_gram_hi_i8 forms the product again) stays behind TUNE["GRAM_TWICE"].  These tests hold the two forms against
each other, bit for bit, in every state the header can be left in:
  (a)  level 1 takes the digit under eagle_set_scan_budget(5e-7) -- the fused kernel has written the level-2 fields and E_hi by then, and
       the header must read as if nobody had (zeros);
  (b)  level 1 declines under the default tight-first budget and level 2 takes the digit (E_hi compared too);
  (b') level 2 runs but it is level 1's bound that passes, at the default budget;
  (c)  a forced digit count: no spectral bound, the slice area holds live digits only.
Operands are built on the host (numpy) so that each case is reached; the case is asserted from the header's `level` field and from what
was written to the spare slot, so a test cannot pass without the fused branch having run.  n_pad = 512 (n = 300): one diagonal tile pair per
panel, one mirrored off-diagonal pair, padding rows; n_pad = 768 (n = 700): three row panels."""
import ctypes as C

import numpy as np
import pytest

from eagleeverything_amd._lib import TUNE

from exact_lastdigit import decode_header as _hdr   # the head of the digit workspace, decoded in one place

pytestmark = pytest.mark.gpu
L_MARKERS = 256
POISON = 0xA5
TWO_KERNELS = TUNE["GRAM_TWICE"]   # level 2 forms Ds Ds again


def _operands(n, diag):
    """W = diag(diag * U(0.8, 1.2)) + a symmetric N(0, 1e-3^2) off-diagonal part, v, and genotypes in {-1, 0, +1}."""
    rng = np.random.default_rng(7)
    E = rng.standard_normal((n, n)) * 1e-3
    W = np.diag(diag * (0.8 + 0.4 * rng.random(n))) + 0.5 * (E + E.T)
    v = rng.standard_normal(n)
    Mt8 = rng.integers(-1, 2, size=(L_MARKERS, n)).astype(np.int8)
    return W, v, Mt8


def _run(torch, sh, tune):
    """prepare + scan on a poisoned workspace: (header bytes, {slot: bytes}, vara)."""
    ws = sh._ws()
    ws.fill_(POISON)
    sh.L.eagle_dev_set_tune(sh.ctx, tune)
    try:
        sh.scan_operands()
        sh.vara_prepare()
        torch.cuda.synchronize()
        head = ws[:256].cpu().numpy().copy()
        nslots = C.c_int(0)
        n2 = sh.np_ * sh.np_
        slots = {}
        for k in range(int(sh.nslices) if sh.nslices else 7):
            off = int(sh.L.eagle_vara_i8_ws_slot_offset(sh.np_, sh.Lp, int(sh.nslices), k, C.byref(nslots)))
            slots[k] = ws[off:off + n2].cpu().numpy().copy()
        assert nslots.value == len(slots)
        sh.vara_kernel()
        sh.certify()
        torch.cuda.synchronize()
        return head, slots, sh.vara[:L_MARKERS].cpu().numpy().copy()
    finally:
        sh.L.eagle_dev_set_tune(sh.ctx, TUNE["SHIPPED"])


# diag: the scale of W's diagonal that reaches the case at both sizes (the digit rule restated on the host, as tests/test_gpu_spectral.py
# does, gives level 2 for 0.05 .. 0.065 and level 1 from 0.07 on at these operands)
CASES = {"a": (0.2, 5e-7, 0), "b": (0.058, 0.0, 0), "b1": (0.2, 0.0, 0), "c": (0.058, 0.0, 4)}


@pytest.mark.parametrize("n", [300, 700])
@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_gram_leaves_what_the_two_kernels_leave(n, case):
    import torch
    from eagleeverything_amd.sharded import DeviceShard
    diag, budget, nslices = CASES[case]
    W, v, Mt8 = _operands(n, diag)
    sh = DeviceShard(n, L_MARKERS)
    assert sh.np_ == {300: 512, 700: 768}[n]
    sh.Mt8[:L_MARKERS, :n] = torch.from_numpy(Mt8).to(sh.dev)
    sh.set_W(W, v)
    sh.mode, sh.nslices = 1, nslices
    sh._check(sh.L.eagle_set_scan_budget(sh.ctx, budget))
    try:
        head2, slots2, vara2 = _run(torch, sh, TWO_KERNELS)
        head1, slots1, vara1 = _run(torch, sh, TUNE["SHIPPED"])
    finally:
        sh._check(sh.L.eagle_set_scan_budget(sh.ctx, 0.0))
    h1, h2 = _hdr(head1), _hdr(head2)
    print(case, n, "fused", h1, "two kernels", h2)
    assert np.array_equal(head1, head2), (h1, h2)
    assert np.array_equal(vara1, vara2) and np.all(np.isfinite(vara1))
    S_cut = h1["S_sliced"]
    for k in range(S_cut):   # every live digit slice
        assert np.array_equal(slots1[k], slots2[k]), k
    spare = len(slots1) - 2
    untouched = lambda x: bool(np.all(x == POISON))
    if case == "a":      # level 1 took the digit at once: the fused form has been through the level-2 side, and the header does not show it
        assert (h1["level"], h1["S"], h1["budget"]) == (1, S_cut - 1, 5e-7) and S_cut < spare + 1
        assert (h1["lo_sumsq"], h1["maxdiag"], h1["hi_overflow"], h1["spec_try2"]) == (0, 0, 0, 0)
        assert untouched(slots2[spare]) and not untouched(slots1[spare])
    elif case in ("b", "b1"):   # level 2 ran
        assert (h1["level"], h1["S"]) == (2 if case == "b" else 1, S_cut - 1)
        assert h1["lo_sumsq"] > 0 and h1["maxdiag"] > 0 and h1["hi_overflow"] == 0 and h1["spec_try2"] == 0
        assert np.array_equal(slots1[spare], slots2[spare]) and not untouched(slots1[spare])
        E = slots1[spare].view(np.int8).reshape(sh.np_, sh.np_)
        assert np.array_equal(E, E.T) and not E.diagonal().any() and E[:n, :n].any() and not E[n:].any()
    else:                # forced count: no spectral bound, nothing beyond the digits asked for
        assert (h1["level"], h1["S"], S_cut) == (0, 4, 4) and len(slots1) == 4
        assert (h1["lo_sumsq"], h1["maxdiag"], h1["hi_overflow"], h1["spec_try2"]) == (0, 0, 0, 0)
