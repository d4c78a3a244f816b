"""CPU: the C ABI of the runs of homozygosity without a device -- eagle_roh and eagle_bed_roh are declared, exported and bound, section
1b'''vi of the header states the rule and what is not claimed, and every argument error is decided before a context is needed
(ctx == NULL: the text comes through eagle_open_error).  The HIP-free pieces behind them (csrc/eagle_host.h: roh_arg_error,
roh_block_table, roh_pos_check, roh_offsets) also run in a stand-alone program under ASan + UBSan, built as tests/test_host_sanitizers.py
builds its source.  No device work."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG = -3
NAMES = ("eagle_roh", "eagle_bed_roh")


def header():
    return open(os.path.join(ROOT, "include", "eagle_hip.h")).read()


def test_roh_symbols_declared_exported_and_bound():
    from eagleeverything_amd import _lib, rcpp_api
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, txt), name + " is not declared in include/eagle_hip.h"
        assert hasattr(L, name), "libeaglehip.so does not export " + name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
    assert len(_lib.SIGNATURES["eagle_roh"][1]) == 11 and len(_lib.SIGNATURES["eagle_bed_roh"][1]) == 12
    m = re.search(r"typedef struct eagle_roh_params \{\s*int64_t ([^;]*);", txt)
    assert m and tuple(f.strip() for f in m.group(1).split(",")) == tuple(f for f, _ in _lib.RohParams._fields_) == rcpp_api._ROH_FIELDS
    assert C.sizeof(_lib.RohParams) == 72
    assert re.search(r"#define EAGLE_ROH_CHUNK 1024L", txt) and re.search(r"#define EAGLE_ROH_MAX_WINDOW 64L", txt)
    ctxh = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_ctx.h")).read()
    for name in ("eagle_dev_roh_flags_i8", "eagle_dev_roh_flags_bed", "eagle_dev_roh_segments"):
        assert re.search(r"\bint\s+%s\s*\(\s*eagle_ctx\s*\*" % name, ctxh) and hasattr(L, name)
    makefile = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "Makefile")).read()
    assert "eagle_roh.hip" in makefile and "eagle_roh.o" in makefile
    kern = open(os.path.join(ROOT, "eagleeverything_amd", "csrc", "eagle_roh.hip")).read()
    assert "k_roh_flags" in kern and "k_roh_segments" in kern and "asm" not in re.sub(r"//.*", "", kern)


def test_header_states_the_rule_and_what_is_not_claimed():
    txt = " ".join(header().replace("*", " ").split())
    sec = txt[txt.index("1b'''vi."):txt.index("1b''''.")]
    for phrase in ("PLINK --homozyg AS DOCUMENTED", "neither claimed nor tested", "hom: image value +-1, .bed codes 00 and 11",
                   "miss: .bed code 01 only", "a missing call of the original data is a het", "maximal run of panel markers with equal chrom[m]",
                   "NULL: pos[m] = m", "non-decreasing inside every block", "1 <= w <= 64", "a <= s and s + w <= e",
                   "<= win_het and its miss count is <= win_miss", "hom >= 1 and hom 65536 >= thr16 cover", "0 <= thr16 <= 65536",
                   "A block shorter than w has no flagged marker", "pos[m + 1] - pos[m] > max_gap", "nsnp = e - s + 1 >= min_snp",
                   "len = pos[e] - pos[s] >= min_len", "len <= max_density nsnp", "max_density <= 2^31", "max_het < 0 or nhet <= max_het",
                   "n x 4 int64", "(individual, s, e, nhet, nmiss, block ordinal)", "sorted by (individual, s)", "nseg_out is always the total",
                   "untouched otherwise", "returns EAGLE_OK either way", "n <= 0x3fffffff", "EAGLE_ERR_NOMEM, decided before any kernel runs",
                   "does not depend on the window size", "decided before the context is used"):
        assert phrase in sec, phrase
    assert txt.index("1b'''v.") < txt.index("1b'''vi.") < txt.index("1b''''.")
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "Runs of homozygosity" in readme and "PLINK program itself is neither claimed nor tested" in readme


def test_roh_interface_is_public():
    from eagleeverything_amd import r_api, rcpp_api
    for name in ("roh_host", "roh_classes_mt8", "roh_classes_bed", "roh_incidence", "roh_summary", "ROH"):
        assert callable(getattr(r_api, name))
    p = inspect.signature(r_api.ROH).parameters
    assert [(k, p[k].default) for k in list(p)[1:14]] == [
        ("map", None), ("bed", None), ("include", None), ("window", 50), ("window_het", 1), ("window_missing", 5), ("threshold", 0.05),
        ("min_snp", 100), ("min_kb", 1000), ("max_density_kb", 50), ("max_gap_kb", 1000), ("max_het", None), ("availmemGb", 8)]
    assert list(inspect.signature(r_api.roh_host).parameters) == ["classes", "chrom", "pos", "params"]
    assert list(inspect.signature(r_api.roh_incidence).parameters) == ["seg", "L"]
    p = inspect.signature(rcpp_api.roh).parameters
    assert list(p)[:4] == ["f_name_ascii_Mt", "dims", "chrom", "pos"] and p["chrom"].default is None and p["pos"].default is None
    p = inspect.signature(rcpp_api.bed_roh).parameters
    assert list(p)[:5] == ["bed_path", "dims", "include", "chrom", "pos"] and p["include"].default is None
    assert rcpp_api.ROH_DEFAULTS["thr16"] == r_api.roh_thr16(0.05) == int(0.05 * 65536 + 0.5) == 3277
    assert r_api.roh_thr16(0.0) == 0 and r_api.roh_thr16(1.0) == 65536 and r_api.roh_thr16(0.5) == 32768


def params(**kw):
    from eagleeverything_amd import _lib, rcpp_api
    p = dict(rcpp_api.ROH_DEFAULTS)
    p.update(kw)
    return _lib.RohParams(*[p[f] for f in rcpp_api._ROH_FIELDS])


def test_c_argument_errors_need_no_context(tmp_path):
    from eagleeverything_amd import _lib
    L = _lib.load()

    def text():
        return L.eagle_open_error().decode()

    nm, n = 7, 5
    dims = (C.c_long * 2)(n, nm)
    ind, seg, total = (C.c_int64 * (4 * n))(), (C.c_int32 * (6 * 8))(), C.c_long(0)
    chrom, pos = (C.c_int32 * nm)(1, 1, 1, 2, 2, 3, 3), (C.c_int64 * nm)(10, 20, 30, 5, 6, 1, 1)

    def ref(p):
        return C.cast(C.pointer(p), C.c_void_p)

    for fn, who, good, names in (
            (L.eagle_roh, "roh", (str(tmp_path / "Mt.ascii").encode(), dims, chrom, pos, ref(params()), 8.0, ind, seg, 8, C.byref(total)),
             ("path", "dims", "chrom", "pos", "prm", "mem", "ind", "seg", "cap", "total")),
            (L.eagle_bed_roh, "bed_roh", (str(tmp_path / "p.bed").encode(), dims, None, chrom, pos, ref(params()), 8.0, ind, seg, 8, C.byref(total)),
             ("path", "dims", "include", "chrom", "pos", "prm", "mem", "ind", "seg", "cap", "total"))):

        def call(**kw):
            return fn(None, *[kw.get(k, v) for k, v in zip(names, good)])
        assert call(path=None) == ERR_ARG and text().startswith(who + ":") and "NULL" in text()
        assert call(dims=None) == ERR_ARG and "NULL" in text()
        assert call(prm=None) == ERR_ARG and "NULL" in text()
        assert call(ind=None) == ERR_ARG and "NULL" in text()
        assert call(total=None) == ERR_ARG and "NULL" in text()
        assert call(seg=None) == ERR_ARG and "seg_out" in text()                        # seg_cap > 0 needs the buffer
        assert call(cap=-1) == ERR_ARG and "seg_cap" in text()
        assert call(dims=(C.c_long * 2)(0, nm)) == ERR_ARG and "dims" in text()
        assert call(dims=(C.c_long * 2)(n, -1)) == ERR_ARG and "dims" in text()
        assert call(dims=(C.c_long * 2)(n, 1 << 31), chrom=None, pos=None, include=None) == ERR_ARG and "2^31" in text()
        for kw, word in ((dict(w=0), "w must be in [1, 64]"), (dict(w=65), "w must be in [1, 64]"), (dict(win_het=-1), "win_het"),
                         (dict(win_miss=-1), "win_miss"), (dict(thr16=-1), "thr16"), (dict(thr16=65537), "thr16"), (dict(min_snp=0), "min_snp"),
                         (dict(min_len=-1), "min_len"), (dict(max_gap=-1), "max_gap"), (dict(max_density=-1), "max_density"),
                         (dict(max_density=(1 << 31) + 1), "max_density")):
            assert call(prm=ref(params(**kw))) == ERR_ARG and word in text() and text().startswith(who + ":"), kw
        assert call(pos=(C.c_int64 * nm)(10, 20, 19, 5, 6, 1, 1)) == ERR_ARG and "pos decreases inside a block (panel marker 2)" in text()
        assert call(pos=(C.c_int64 * nm)(10, 20, 30, 5, 6, 1, 0)) == ERR_ARG and "panel marker 6" in text()
        assert call(chrom=None) == ERR_ARG and "panel marker 3" in text()              # one block: the chromosome edges now count
        # what passes the rule stops at the missing context
        assert call() == ERR_ARG and "no context" in text()
        assert call(chrom=None, pos=None, seg=None, cap=0) == ERR_ARG and "no context" in text()
        assert call(prm=ref(params(w=64, thr16=65536, max_density=1 << 31, max_het=5, win_het=1000))) == ERR_ARG and "no context" in text()
        assert call(prm=ref(params(w=1, thr16=0, min_snp=1))) == ERR_ARG and "no context" in text()

    # the .bed entry point's own
    fn = L.eagle_bed_roh
    good = (str(tmp_path / "p.bed").encode(), dims, None, None, None, ref(params()), 8.0, ind, seg, 8, C.byref(total))
    names = ("path", "dims", "include", "chrom", "pos", "prm", "mem", "ind", "seg", "cap", "total")

    def call(**kw):
        return fn(None, *[kw.get(k, v) for k, v in zip(names, good)])
    assert call(dims=(C.c_long * 2)(1 << 30, nm)) == ERR_ARG and "2^30" in text()
    assert call(include=(C.c_uint8 * nm)()) == ERR_ARG and "no marker" in text()
    inc = (C.c_uint8 * nm)(1, 0, 1, 1, 0, 0, 0)
    assert call(include=inc, pos=(C.c_int64 * 3)(3, 2, 1)) == ERR_ARG and "panel marker 1" in text()        # pos is by PANEL marker
    assert call(include=inc, pos=(C.c_int64 * 3)(3, 2, 1), chrom=(C.c_int32 * 3)(1, 2, 3)) == ERR_ARG and "no context" in text()


def test_python_wrappers_refuse_before_the_library(tmp_path):
    from eagleeverything_amd import rcpp_api
    Mt, bed = str(tmp_path / "Mt.ascii"), str(tmp_path / "a.bed")
    for kw in (dict(chrom=[1, 1, 2]), dict(chrom=[1, 1.5, 2, 2, 2, 2]), dict(pos=[1, 2, 3]), dict(pos=[1, 2, 3, 4, 5, 6.5]),
               dict(pos=[1, 2, 3, 2, 5, 6]), dict(chrom=[1, 1, 1, 2, 2, 2], pos=[1, 2, 3, 1, 2, 1]), dict(w=0), dict(w=65), dict(w=2.5),
               dict(win_het=-1), dict(win_miss=-1), dict(thr16=65537), dict(thr16=-1), dict(min_snp=0), dict(min_len=-1), dict(max_gap=-1),
               dict(max_density=-1), dict(max_density=(1 << 31) + 1), dict(window=50), dict(seg_cap=-1), dict(max_het="x")):
        with pytest.raises(ValueError):
            rcpp_api.roh(Mt, (4, 6), **kw)
        with pytest.raises(ValueError):
            rcpp_api.bed_roh(bed, (4, 6), **kw)
    with pytest.raises(ValueError):
        rcpp_api.bed_roh(bed, (4, 6), include=[1, 0, 1])
    with pytest.raises(ValueError):
        rcpp_api.bed_roh(bed, (4, 6), include=[1, 0, 1, 0, 1, 0], chrom=np.zeros(6))                  # chrom is by PANEL marker
    p = rcpp_api.roh_params(w=7, max_het=-9)
    assert p["w"] == 7 and p["max_het"] == -9 and p["win_miss"] == 5
    assert rcpp_api.roh_blocks([5, 5, 2, 2, 2, 5], 6).tolist() == [0, 2, 5, 6] and rcpp_api.roh_blocks(None, 6).tolist() == [0, 6]


def test_roh_host_pieces_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "roh_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_roh_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "roh host checks passed" in r.stdout
