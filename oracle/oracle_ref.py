"""ctypes binding of oracle/_ref/libeagle_ref.so and libeagle_ref_ld.so: the reference's own src/*.cpp compiled unmodified on
the stand-in headers of oracle/refstub/ (oracle/Makefile, target `ref`; built by __graft_entry__.build() when the reference
checkout is present).  TEST INFRASTRUCTURE ONLY.

Same call shapes as oracle_c, so a test can run one next to the other.  Every function takes ld=False; ld=True runs the build
whose products accumulate in long double (the high-precision reference for fp64 outputs).  messages() returns what the
reference passed to message() during the last call, one string per call, arguments pasted without a separator.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SO = {False: os.path.join(_HERE, "_ref", "libeagle_ref.so"), True: os.path.join(_HERE, "_ref", "libeagle_ref_ld.so")}
_libs = {}
_last = []

c_dp = C.POINTER(C.c_double)
c_lp = C.POINTER(C.c_long)
c_ip = C.POINTER(C.c_int)


class ReferenceError_(RuntimeError):
    """Rcpp::stop in the reference (code -1), or an access the reference leaves undefined that the stand-in refused (-2)."""

    def __init__(self, code, text):
        super().__init__(text)
        self.code, self.text = code, text


OracleError = ReferenceError_


def reference_src():
    """The reference's src directory: EAGLE_REFERENCE_SRC (relative names count from the repository root)."""
    p = os.environ.get("EAGLE_REFERENCE_SRC", os.path.join("..", "reference", "MyPackage", "Eagle", "src"))
    return p if os.path.isabs(p) else os.path.normpath(os.path.join(_ROOT, p))


def sources_present():
    return os.path.isfile(os.path.join(reference_src(), "ReadBlock.cpp"))


def available():
    return all(os.path.exists(p) for p in _SO.values())


def lib(ld=False):
    if ld not in _libs:
        if not os.path.exists(_SO[ld]):
            raise RuntimeError("%s is missing: run build()" % os.path.relpath(_SO[ld], _ROOT))
        L = C.CDLL(_SO[ld])
        L.er_last_error.restype = C.c_char_p
        L.er_message.restype = C.c_char_p
        L.er_message.argtypes = [C.c_long]
        L.er_message_count.restype = C.c_long
        L.er_clear_messages.restype = None
        L.er_ReadBlock.argtypes = [C.c_char_p, C.c_long, C.c_long, C.c_long, c_dp]
        L.er_calculateMMt.argtypes = [C.c_char_p, C.c_double, C.c_int, c_dp, C.c_long, C.c_long, C.c_long, C.c_int, c_dp]
        L.er_calculate_a_and_vara.argtypes = [C.c_char_p, c_dp, C.c_long, c_dp, c_dp, C.c_double, C.c_long, C.c_long, c_dp, C.c_int,
                                              c_dp, c_dp, c_lp]
        L.er_calculate_reduced_a.argtypes = [C.c_char_p, C.c_double, c_dp, c_dp, C.c_double, C.c_long, C.c_long, c_dp, C.c_long,
                                             C.c_int, c_dp, c_lp]
        L.er_extract_geno.argtypes = [C.c_char_p, C.c_double, C.c_long, C.c_long, C.c_long, c_ip]
        L.er_getRowColumn.argtypes = [C.c_char_p, c_lp]
        L.er_createM_ASCII.argtypes = [C.c_char_p] * 6 + [C.c_double, C.c_long, C.c_long, C.c_int, C.c_char_p, c_ip]
        L.er_CreateASCIInospace.argtypes = [C.c_char_p, C.c_char_p, C.c_long, C.c_long, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int,
                                            C.c_char_p, c_ip]
        L.er_CreateASCIInospace_PLINK.argtypes = [C.c_char_p, C.c_char_p, C.c_long, C.c_long, C.c_int, c_ip]
        L.er_createMt_ASCII.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_double, C.c_long, C.c_long, C.c_int]
        L.er_ReshapeM.argtypes = [C.c_char_p, C.c_char_p, c_lp, C.c_long, C.c_long, C.c_long, c_lp]
        assert bool(L.er_acc_is_long_double()) == ld
        _libs[ld] = L
    return _libs[ld]


def messages():
    """message() lines of the last call into the reference (either build)."""
    return list(_last)


def _call(ld, name, *args, message=None):
    L = lib(ld)
    L.er_clear_messages()
    rc = getattr(L, name)(*args)
    _last[:] = [L.er_message(i).decode() for i in range(L.er_message_count())]
    if message is not None:
        for m in _last:
            message(m)
    if rc != 0:
        raise ReferenceError_(rc, L.er_last_error().decode())


def _dp(a):
    return a.ctypes.data_as(c_dp)


def _f64(a):
    return np.require(np.asarray(a, dtype=np.float64), requirements=["ALIGNED", "WRITEABLE", "F"])


def _sel(selected_loci):
    s = np.atleast_1d(np.asarray(selected_loci, dtype=np.float64)).copy()
    return s, _dp(s), s.size


def ReadBlock(asciifname, start_row, numcols, numrows_in_block, ld=False):
    out = np.zeros((numrows_in_block, numcols), dtype=np.float64, order="F")
    _call(ld, "er_ReadBlock", os.fsencode(asciifname), start_row, numcols, numrows_in_block, _dp(out))
    return out


def calculateMMt_rcpp(f_name_ascii, max_memory_in_Gbytes, num_cores, selected_loci, dims, quiet=True, message=None,
                      return_branch=False, ld=False):
    """return_branch: rows per block as the reference announced it ("number of rows in block is N"), 0 for the in-memory branch."""
    n, L = int(dims[0]), int(dims[1])
    s, sp, ns = _sel(selected_loci)
    out = np.zeros((n, n), dtype=np.float64, order="F")
    _call(ld, "er_calculateMMt", os.fsencode(f_name_ascii), float(max_memory_in_Gbytes), int(num_cores), sp, ns, n, L,
          int(bool(quiet)), _dp(out), message=message)
    if not return_branch:
        return out
    rows = [m for m in _last if m.startswith("number of rows in block is ")]
    return out, (int(rows[0].rsplit(" ", 1)[1]) if rows else 0)


def calculate_a_and_vara_rcpp(f_name_ascii, selected_loci, inv_MMt_sqrt, dim_reduced_vara, max_memory_in_Gbytes, dims, a,
                              quiet=True, message=None, return_branch=False, ld=False):
    """return_branch: the number of "Performing block iteration ... i" lines, i.e. the number of blocks; 0 = in-memory branch."""
    L, n = int(dims[0]), int(dims[1])
    S, V, ah = _f64(inv_MMt_sqrt), _f64(dim_reduced_vara), _f64(np.ravel(a))
    s, sp, ns = _sel(selected_loci)
    a_out, v_out, ln = np.zeros(L), np.zeros(L), C.c_long(-1)
    _call(ld, "er_calculate_a_and_vara", os.fsencode(f_name_ascii), sp, ns, _dp(S), _dp(V), float(max_memory_in_Gbytes), L, n,
          _dp(ah), int(bool(quiet)), _dp(a_out), _dp(v_out), C.byref(ln), message=message)
    if ln.value != L:  # the sentinel List(a=0, vara=0)
        res = {"a": a_out[: ln.value].copy(), "vara": v_out[: ln.value].copy()}
    else:
        res = {"a": a_out.reshape(L, 1), "vara": v_out.reshape(L, 1)}
    nblocks = sum(m.startswith("Performing block iteration ... ") for m in _last)
    return (res, nblocks) if return_branch else res


def calculate_reduced_a_rcpp(f_name_ascii, varG, P, y, max_memory_in_Gbytes, dims, selected_loci, quiet=True, message=None,
                             ld=False):
    n, L = int(dims[0]), int(dims[1])
    Pm, yv = _f64(P), _f64(np.ravel(y))
    s, sp, ns = _sel(selected_loci)
    out, ln = np.zeros(max(L, 1)), C.c_long(-1)
    _call(ld, "er_calculate_reduced_a", os.fsencode(f_name_ascii), float(varG), _dp(Pm), _dp(yv), float(max_memory_in_Gbytes), n, L,
          sp, ns, int(bool(quiet)), _dp(out), C.byref(ln), message=message)
    return out[: ln.value].reshape(ln.value, 1).copy()


def extract_geno_rcpp(f_name_ascii, max_memory_in_Gbytes, selected_locus, dims, ld=False):
    n, L = int(dims[0]), int(dims[1])
    out = np.zeros(n, dtype=np.int32)
    _call(ld, "er_extract_geno", os.fsencode(f_name_ascii), float(max_memory_in_Gbytes), int(selected_locus), n, L,
          out.ctypes.data_as(c_ip))
    return out


def getRowColumn(fname, ld=False):
    d = (C.c_long * 2)()
    _call(ld, "er_getRowColumn", os.fsencode(fname), d)
    return [int(d[0]), int(d[1])]


def createM_ASCII_rcpp(f_name, f_name_ascii, type, AA, AB, BB, max_memory_in_Gbytes, dims, quiet=True, message=None,
                       missing="NA", ld=False):
    """-> (it_worked, messages)."""
    ok = C.c_int(-1)
    enc = lambda v: str(v).encode()
    _call(ld, "er_createM_ASCII", os.fsencode(f_name), os.fsencode(f_name_ascii), enc(type), enc(AA), enc(AB), enc(BB),
          float(max_memory_in_Gbytes), int(dims[0]), int(dims[1]), int(bool(quiet)), enc(missing), C.byref(ok), message=message)
    return bool(ok.value), messages()


def CreateASCIInospace(fname, asciifname, dims, AA, AB, BB, quiet=True, message=None, missing="NA", ld=False):
    ok = C.c_int(-1)
    enc = lambda v: str(v).encode()
    _call(ld, "er_CreateASCIInospace", os.fsencode(fname), os.fsencode(asciifname), int(dims[0]), int(dims[1]), enc(AA), enc(AB),
          enc(BB), int(bool(quiet)), enc(missing), C.byref(ok), message=message)
    return bool(ok.value), messages()


def CreateASCIInospace_PLINK(fname, asciifname, dims, quiet=True, message=None, ld=False):
    ok = C.c_int(-1)
    _call(ld, "er_CreateASCIInospace_PLINK", os.fsencode(fname), os.fsencode(asciifname), int(dims[0]), int(dims[1]),
          int(bool(quiet)), C.byref(ok), message=message)
    return bool(ok.value), messages()


def createMt_ASCII_rcpp(f_name, f_name_ascii, type, max_memory_in_Gbytes, dims, quiet=True, message=None, ld=False):
    _call(ld, "er_createMt_ASCII", os.fsencode(f_name), os.fsencode(f_name_ascii), str(type).encode(), float(max_memory_in_Gbytes),
          int(dims[0]), int(dims[1]), int(bool(quiet)), message=message)


def ReshapeM_rcpp(fnameM, fnameMt, indxNA, dims, ld=False):
    na = np.ascontiguousarray(np.atleast_1d(np.asarray(indxNA, dtype=np.int64)).ravel(), dtype=np.int64)
    out = (C.c_long * 2)()
    _call(ld, "er_ReshapeM", os.fsencode(fnameM), os.fsencode(fnameMt), na.ctypes.data_as(c_lp), na.size, int(dims[0]), int(dims[1]),
          out)
    return [int(out[0]), int(out[1])]


def tsq_argmax(a, vara):
    """find_qtl.R:71-83 is R code, which no build of src/*.cpp covers; this is oracle_c's rule, kept here so call sites read alike."""
    from oracle import oracle_c
    return oracle_c.tsq_argmax(a, vara)
