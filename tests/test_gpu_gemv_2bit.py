"""The genotype pass from the 2-bit image (csrc/eagle_kernels.hip: k_pack_2bit, k_gemv_mfma_2bit; eagle_dev_vara_i8_prepare_packed).

The pass computes exact int32 MFMA sums over the genotype bytes; the 2-bit image decodes to those bytes, so every output must equal the
int8 pass's bit for bit.  Shapes: n_pad = 256 (n = 200: one 256-column super-step, the last 16-byte group ragged) and n_pad = 5376 (past
the 5,120-column sweep of the three-vector form: the second sweep adds into the outputs); L_pad = 16 (one marker group) and 272 (17 groups:
more than the 16 waves of a block).  Rows of all -1, all +1 and zeros ride along in every image."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SHAPES = [(200, 256), (5300, 5376)]
L_PADS = [16, 272]
_IMAGES = {}


def _image(n, n_pad, L_pad):
    """Genotypes in {-1, 0, +1}, zero from column n on; made once per shape and left as it is."""
    key = (n, n_pad, L_pad)
    if key not in _IMAGES:
        rng = np.random.default_rng(1000 * n_pad + L_pad)
        M = np.zeros((L_pad, n_pad), dtype=np.int8)
        M[:, :n] = rng.integers(-1, 2, size=(L_pad, n))
        M[0, :n], M[1, :n], M[2, :] = -1, 1, 0
        M[L_pad - 1, :n] = -1
        M[L_pad - 2, :n] = 1
        vecs = rng.standard_normal((3, n_pad)) * np.exp(rng.uniform(-12, 12, size=(3, n_pad)))   # padding entries too: they meet zeros
        _IMAGES[key] = (M, vecs)
    return _IMAGES[key]


def _ctx():
    import torch
    from eagleeverything_amd import _lib, rcpp_api
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    return torch, lib, rcpp_api.context(0), dev, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("L_pad", L_PADS)
@pytest.mark.parametrize("n,n_pad", SHAPES)
def test_pack_decodes_to_the_int8_image_and_the_pass_gives_the_same_bits(n, n_pad, L_pad):
    torch, lib, ctx, dev, stream = _ctx()
    M, vecs = _image(n, n_pad, L_pad)
    Mt8 = torch.from_numpy(M).to(dev)
    Mt2 = torch.full((L_pad, n_pad // 4), 0xA5, dtype=torch.uint8, device=dev)
    assert lib.eagle_dev_pack_2bit(ctx, Mt8.data_ptr(), L_pad, n_pad, n_pad, Mt2.data_ptr(), stream) == 0
    back = torch.full_like(Mt8, 7)
    assert lib.eagle_dev_unpack_2bit(ctx, Mt2.data_ptr(), L_pad, n_pad, n_pad, back.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(back, Mt8)
    # the layout rule restated: genotype k of a marker is the code m & 3 at bits 8 b + 2 d of dword 16 T + 4 q + u of its packed row,
    # T = k >> 8, u = (k >> 6) & 3, q = (k >> 4) & 3, d = (k >> 2) & 3, b = k & 3
    k = np.arange(n_pad)
    word, bit = 16 * (k >> 8) + 4 * ((k >> 4) & 3) + ((k >> 6) & 3), 8 * (k & 3) + 2 * ((k >> 2) & 3)
    words = Mt2.cpu().numpy().view(np.uint32)
    assert np.array_equal((words[:, word] >> bit.astype(np.uint32)) & 3, M.astype(np.uint8) & 3)
    v, w, x = (torch.from_numpy(vecs[i].copy()).to(dev) for i in range(3))
    # three vectors (two sweeps of 5,120 columns at n_pad = 5376), two vectors, one vector, and a and x without the squared term
    for form in ((v, w, x), (v, w, None), (v, None, None), (v, None, x)):
        outs = []
        for fn, img in ((lib.eagle_dev_gemv3_i8, Mt8), (lib.eagle_dev_gemv3_2bit, Mt2)):
            o = [torch.full((L_pad,), float("nan"), dtype=torch.float64, device=dev) if t is not None else None for t in form]
            assert fn(ctx, img.data_ptr(), L_pad, n_pad, n_pad, _ptr(form[0]), _ptr(form[1]), _ptr(form[2]), 0.5, _ptr(o[0]), _ptr(o[1]), _ptr(o[2]),
                      stream) == 0
            torch.cuda.synchronize()
            outs.append([None if t is None else t.cpu().numpy() for t in o])
        for name, a8, a2 in zip("adx", outs[0], outs[1]):
            if a8 is not None:
                assert np.all(np.isfinite(a8)) and np.array_equal(a8, a2), (name, [t is not None for t in form])
    # and the int8 pass is the product it claims to be (fp64 reference on the host; the digits carry 62 bits of the largest entry)
    ref = 0.5 * (M.astype(np.float64) @ vecs[0])
    np.testing.assert_allclose(outs[0][0], ref, rtol=0, atol=1e-12 * np.abs(vecs[0]).max() * n_pad)


def test_vara_prepare_gives_the_same_bits_with_the_packed_image_on_and_off():
    import torch
    from eagleeverything_amd.sharded import DeviceShard
    n, L = 300, 512
    rng = np.random.default_rng(3)
    E = rng.standard_normal((n, n)) * 1e-3
    W = np.diag(0.5 * (0.8 + 0.4 * rng.random(n))) + 0.5 * (E + E.T)
    sh = DeviceShard(n, L)
    sh.Mt8[:L, :n] = torch.from_numpy(rng.integers(-1, 2, size=(L, n)).astype(np.int8)).to(sh.dev)
    sh.set_W(W, rng.standard_normal(n))
    sh.mode = 1
    got = {}
    for packed in (False, True):
        sh.packed = packed
        sh._ws().fill_(0xA5)
        sh.a.fill_(float("nan"))
        sh.scan_operands()
        sh.vara_prepare()
        torch.cuda.synchronize()
        assert (sh.Mt2 is not None) == packed
        ws = sh.ws.cpu().numpy().copy()   # a's neighbours of the pass, the diagonal term and m^T rho, lie in the workspace
        sh.vara_kernel()
        sh.certify()
        sh.argmax()
        torch.cuda.synchronize()
        got[packed] = (sh.a[:L].cpu().numpy().copy(), sh.vara[:L].cpu().numpy().copy(), ws, sh.best())
    for k in range(3):
        assert np.array_equal(got[False][k], got[True][k]), k
    assert got[False][3] == got[True][3] and np.all(np.isfinite(got[True][0]))
    # new genotypes: the image goes with the re-centred one
    sh.Mt8s = None
    assert sh.Mt2 is None
