"""CPU: the argument errors of eagle_weighted_gram (include/eagle_hip.h section 1b'''') are decided before a context is needed: with
ctx == NULL each returns EAGLE_ERR_ARG and leaves its text in eagle_open_error().  No device work."""
import ctypes as C

import numpy as np

ERR_ARG = -3
U32P = C.POINTER(C.c_uint32)
I64P = C.POINTER(C.c_int64)


def test_weighted_gram_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()
    fn = L.eagle_weighted_gram
    dims, zero, neg = (C.c_long * 2)(4, 6), (C.c_long * 2)(4, 0), (C.c_long * 2)(-1, 6)
    huge, wrap = (C.c_long * 2)(4, 1 << 31), (C.c_long * 2)(4, 16909321)
    q = (C.c_uint32 * 6)(0, 1, 127, 128, 16384, 2097151)
    out = (C.c_int64 * 16)()
    path = str(tmp_path / "M.ascii").encode()                              # never opened

    def text():
        return L.eagle_open_error().decode()
    assert fn(None, None, dims, q, 8.0, out) == ERR_ARG and "weighted_gram" in text() and "NULL" in text()
    assert fn(None, path, None, q, 8.0, out) == ERR_ARG and "NULL" in text()
    assert fn(None, path, dims, None, 8.0, out) == ERR_ARG and "NULL" in text()
    assert fn(None, path, dims, q, 8.0, None) == ERR_ARG and "NULL" in text()
    assert fn(None, path, zero, q, 8.0, out) == ERR_ARG and "dims" in text()
    assert fn(None, path, neg, q, 8.0, out) == ERR_ARG and "dims" in text()
    assert fn(None, path, huge, q, 8.0, out) == ERR_ARG and "2^31" in text()
    # one marker more than floor((2^31 - 1) / 127): the int32 accumulator of a digit plane could wrap (decided before q is read)
    assert 127 * 16909320 < 2 ** 31 <= 127 * 16909321
    assert fn(None, path, wrap, q, 8.0, out) == ERR_ARG and "16,909,320" in text()
    for k in range(6):
        bad = np.array([0, 1, 127, 128, 16384, 2097151], dtype=np.uint32)
        bad[k] = 1 << 21
        assert fn(None, path, dims, bad.ctypes.data_as(U32P), 8.0, out) == ERR_ARG and "2^21" in text()
    bad[5] = 0xffffffff
    assert fn(None, path, dims, bad.ctypes.data_as(U32P), 8.0, out) == ERR_ARG and "2^21" in text()
    assert fn(None, path, dims, q, 8.0, out) == ERR_ARG and "no context" in text()
