"""The poison hook (EAGLE_HIP_POISON; csrc/eagle_ctx.h "The allocation path"), the part that needs no GPU.

  * tests/host/test_poison_host.cpp: csrc/eagle_host.h's poison_parse -- unset, empty, every byte, 256, garbage -- under ASan + UBSan,
    built as tests/test_bed_host.py builds its source;
  * the rule pinned to the source text: no device or pinned allocation in csrc/ outside the two functions of the allocation path, and
    every row of DESIGN 3a's inventory names a buffer that exists in the sources;
  * the table of cases of tests/test_gpu_poison.py against the public functions of rcpp_api: an entry point without a case fails here.
"""
import inspect
import os
import re
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "test_poison_host.cpp")
CSRC = os.path.join(ROOT, "eagleeverything_amd", "csrc")
ALLOCATORS = ("hipMalloc(", "hipHostMalloc(", "hipMallocAsync(", "hipHostAlloc(", "hipMallocManaged(", "hipExtMallocWithFlags(", "hipMallocPitch(",
              "hipMalloc3D(", "hipMallocFromPoolAsync(")


def test_poison_parse_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "poison_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC,
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "poison host checks passed" in r.stdout


def _sources():
    return {f: open(os.path.join(CSRC, f), encoding="utf-8", errors="replace").read() for f in sorted(os.listdir(CSRC))
            if f.endswith((".h", ".hip", ".cpp"))}


def _code(text):
    """The text without its comments (a comment may speak of hipMalloc)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return "\n".join(line.split("//")[0] for line in text.split("\n"))


def test_every_allocation_goes_through_the_helper():
    found = []
    for f, text in _sources().items():
        for k, line in enumerate(_code(text).split("\n"), 1):
            for a in ALLOCATORS:
                if re.search(r"(?<![A-Za-z0-9_])" + re.escape(a), line):
                    found.append((f, a, line.strip()))
    # the allocation path itself: dev_alloc's hipMalloc and pin_alloc's hipHostMalloc, nothing else anywhere
    assert sorted((f, a) for f, a, _ in found) == [("eagle_ctx.h", "hipHostMalloc("), ("eagle_ctx.h", "hipMalloc(")], found
    ctx_h = _sources()["eagle_ctx.h"]
    assert re.search(r"static inline hipError_t dev_alloc\(void\*\* p, size_t bytes\) \{\s*const hipError_t e = hipMalloc\(p, bytes\);", ctx_h)
    assert re.search(r"static inline hipError_t pin_alloc\(void\*\* p, size_t bytes\) \{\s*const hipError_t e = hipHostMalloc\(p, bytes,", ctx_h)
    # the hook is read at every allocation, not cached, and adds no ABI symbol
    assert "static inline int poison_byte() { return poison_parse(getenv(\"EAGLE_HIP_POISON\")); }" in ctx_h
    assert "POISON" not in open(os.path.join(ROOT, "include", "eagle_hip.h"), encoding="utf-8").read()


def _inventory_rows():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    m = re.search(r"^## 3a\. .*?$(.*?)^## ", text, flags=re.S | re.M)
    assert m, "DESIGN.md has no section 3a"
    rows = [[c.strip() for c in line.strip().strip("|").split("|")] for line in m.group(1).split("\n") if line.startswith("|")]
    head = [r for r in rows if r[0] == "buffer"]
    assert head and all(h == ["buffer", "owner", "kind", "cleared today", "hook fills it", "first write (index, offset, count, flag)"] for h in head)
    return [r for r in rows if r[0] != "buffer" and not set(r[0]) <= set("-: ")]


def test_inventory_names_buffers_that_exist():
    rows = _inventory_rows()
    assert len(rows) >= 60
    code = "\n".join(_sources().values())
    for r in rows:
        assert len(r) == 6, r
        assert r[2] in ("scratch", "state", "scratch / state"), r
        names = re.findall(r"`([^`]+)`", r[0])
        assert names, r
        for name in names:                                                 # `a.b`, `a->b`, `a[0]`: every identifier of the name is in the sources
            for ident in re.findall(r"[A-Za-z_][A-Za-z0-9_]*", name):
                assert re.search(r"(?<![A-Za-z0-9_])" + re.escape(ident) + r"(?![A-Za-z0-9_])", code), (ident, r[0])
        files = re.findall(r"(eagle_\w+\.(?:hip|cpp|h))", r[1])
        assert files and all(os.path.exists(os.path.join(CSRC, f)) for f in files), r


def test_every_entry_point_has_a_case():
    import test_gpu_poison as P
    from eagleeverything_amd import rcpp_api
    public = {name for name, fn in vars(rcpp_api).items()
              if inspect.isfunction(fn) and fn.__module__ == rcpp_api.__name__ and not name.startswith("_")}
    covered = {e for c in P.CASES.values() for e in c.entries}
    assert covered <= public, sorted(covered - public)
    assert P.NOT_DEVICE <= public, sorted(P.NOT_DEVICE - public)
    assert not covered & P.NOT_DEVICE, sorted(covered & P.NOT_DEVICE)
    missing = public - covered - P.NOT_DEVICE
    assert not missing, "rcpp_api entry points without a case in tests/test_gpu_poison.py: %s" % sorted(missing)
    assert any(c.family == "e2e" for c in P.CASES.values())
    for c in P.CASES.values():                                             # every case names its panel and the larger one of the call before it
        assert c.small in P.PANELS and c.big in P.PANELS and c.big != c.small, c.name
