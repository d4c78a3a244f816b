"""The kernel-form switch (eagle_dev_set_tune, EAGLE_HIP_TUNE): one list of names, enum EagleTune of csrc/eagle_ctx.h, mirrored by
_lib.TUNE; a number the list does not hold -- the forms that have left the library had numbers too -- is the shipped form."""
import os
import re

import numpy as np
import pytest

from eagleeverything_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RETIRED = (3, 4, 7) + tuple(range(21, 29))


def _enum_of_header():
    text = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ctx.h")).read()
    body = re.search(r"enum EagleTune \{(.*?)\};", text, re.S).group(1)
    return {name: int(value) for name, value in re.findall(r"\bTUNE_(\w+)\s*=\s*(\d+)\s*,", body)}


def test_names_in_python_are_the_enum_of_the_library():
    assert _enum_of_header() == _lib.TUNE
    assert len(_lib.TUNE) == 11 and len(set(_lib.TUNE.values())) == 11
    assert _lib.TUNE["SHIPPED"] == 0 and _lib.TUNE["SPECTRAL_OFF"] == 29      # the two numbers bench.py passes


def test_known_values_pass_and_all_others_become_the_default():
    L = _lib.load()
    for name, value in _lib.TUNE.items():
        assert L.eagle_tune_known(value) == value, name
    for value in RETIRED + (-1, 1000):
        assert value not in _lib.TUNE.values()
        assert L.eagle_tune_known(value) == 0, value


@pytest.mark.gpu
@pytest.mark.parametrize("retired", [21, 28])      # the four-wave 128 x 128 GEMM and the round-2 fp64 scan kernel had these numbers
def test_retired_number_runs_the_shipped_form(retired):
    """eagle_dev_gemm_f64 at n = 256 on the integer operands of test_dev_gemm_f64_layout, eagle_dev_vara_f64 on one block of 128 markers
    at n_pad = 256: under a retired number the same bits as under the default, not merely close to them."""
    import torch
    from eagleeverything_amd.sharded import DeviceShard
    n, Lb = 256, 128
    sh = DeviceShard(n, Lb)
    rng = np.random.default_rng(n)
    A = rng.integers(-8, 9, size=(n, n)).astype(np.float64)
    B = rng.integers(-8, 9, size=(n, n)).astype(np.float64)
    dA, dB = torch.from_numpy(A).to(sh.dev), torch.from_numpy(B).to(sh.dev)
    Mt8 = torch.from_numpy(rng.integers(-1, 2, size=(Lb, n)).astype(np.int8)).to(sh.dev)
    Wu = torch.from_numpy(np.triu(rng.standard_normal((n, n)))).to(sh.dev)
    out = {}
    try:
        for tune in (_lib.TUNE["SHIPPED"], retired):
            sh.L.eagle_dev_set_tune(sh.ctx, tune)
            dC = torch.zeros((n, n), dtype=torch.float64, device=sh.dev)
            vara = torch.zeros(Lb, dtype=torch.float64, device=sh.dev)
            torch.cuda.synchronize()
            sh._check(sh.L.eagle_dev_gemm_f64(sh.ctx, dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), n, sh._stream()))
            sh._check(sh.L.eagle_dev_vara_f64(sh.ctx, Mt8.data_ptr(), Lb, n, n, Wu.data_ptr(), vara.data_ptr(), sh._stream()))
            torch.cuda.synchronize()
            out[tune] = (dC.cpu().numpy(), vara.cpu().numpy())
    finally:
        sh.L.eagle_dev_set_tune(sh.ctx, _lib.TUNE["SHIPPED"])
    C0, v0 = out[_lib.TUNE["SHIPPED"]]
    np.testing.assert_array_equal(C0, A @ B)
    assert np.abs(v0).max() > 0
    np.testing.assert_array_equal(out[retired][0], C0)
    np.testing.assert_array_equal(out[retired][1], v0)
