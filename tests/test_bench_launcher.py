"""bench.py's launcher plumbing (no GPU needed): `python bench.py --gpus N` without a launcher must start its N ranks as a CHILD
`python -m torch.distributed.run` (never an exec), refuse quickly when the node has fewer GPUs, and `--form abi` is one process.
The GPU half (a two-rank gloo rehearsal through the very same self-spawn path reproduces the one-rank marker) is marked gpu."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env=None, timeout=120):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=timeout)


def test_dry_run_prints_the_child_command():
    r = _run(["--gpus", "4", "--steps", "2", "--warmup", "1", "--dry-run"])
    assert r.returncode == 0, r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])
    cmd = d["child_command"]
    assert d["launcher"] == "self-spawn" and d["n_gpus"] == 4
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(BENCH)
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "2", "--warmup", "1"]  # the ranks get the same arguments, minus --dry-run


def test_one_gpu_and_external_launcher_do_not_spawn():
    d = json.loads(_run(["--dry-run"]).stdout)
    assert "child_command" not in d and d["n_gpus"] == 1
    d = json.loads(_run(["--gpus", "2", "--dry-run"], env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}).stdout)
    assert "child_command" not in d and d["launcher"] == "external"
    d = json.loads(_run(["--gpus", "2", "--form", "abi", "--dry-run"]).stdout)
    assert d["form"] == "abi" and d["devices"] == [0, 1] and "single process" in d["launcher"]


def test_more_gpus_than_the_node_has_fails_fast():
    import torch
    have = torch.cuda.device_count()
    t = time.time()
    r = _run(["--gpus", str(have + 1) if have else "2"])
    assert r.returncode == 3 and "nothing was launched" in r.stderr
    assert r.stdout.strip() == ""
    assert time.time() - t < 60
    r = _run(["--gpus", str(have + 1) if have else "2", "--form", "abi"])
    assert r.returncode == 3 and "GPU(s)" in r.stderr


def test_steps_and_warmup_are_checked_before_anything_starts():
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r = _run(bad + ["--dry-run"])
        assert r.returncode == 2 and "--steps must be >= 1" in r.stderr and r.stdout.strip() == ""


def _load_dump(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_float64_arrays_and_samples_a_large_output(tmp_path):
    """--dump-outputs' writer: every array float64; below the cap the whole of a and vara, above it the same seeded sample of
    markers on every call, with its indices, inside the cap."""
    import bench
    rng = np.random.default_rng(3)
    a, vara = rng.standard_normal(1000), rng.random(1000) + 0.5
    names = bench.dump_outputs(str(tmp_path / "small"), a, vara, 17, 4.25)
    d = _load_dump(str(tmp_path / "small"))
    assert names == sorted(d) == ["a", "selected_marker", "tsqmax", "vara"]
    assert all(x.dtype == np.float64 for x in d.values())
    assert np.array_equal(d["a"], a) and np.array_equal(d["vara"], vara)
    assert d["selected_marker"].tolist() == [17.0] and d["tsqmax"].tolist() == [4.25]
    for k in range(2):   # 1000 markers = 16 KB: a cap of 8 KB forces the sample
        bench.dump_outputs(str(tmp_path / ("big%d" % k)), a, vara, 17, 4.25, cap=8 << 10)
    d0, d1 = _load_dump(str(tmp_path / "big0")), _load_dump(str(tmp_path / "big1"))
    assert sorted(d0) == ["a", "marker_index", "selected_marker", "tsqmax", "vara"]
    assert all(np.array_equal(d0[k], d1[k]) for k in d0)
    idx = d0["marker_index"].astype(np.int64)
    assert 0 < idx.size < 1000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(d0["a"], a[idx]) and np.array_equal(d0["vara"], vara[idx])
    assert sum(os.path.getsize(str(tmp_path / "big0" / f)) for f in os.listdir(str(tmp_path / "big0"))) <= 8 << 10
    assert bench.DUMP_CAP_BYTES == 64 << 20


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_the_timed_step_returned(tmp_path):
    """A plain run prints the headline without the measurements --full adds; its dump is the last timed step's a and vara (the
    selected marker is their first tsq arg-max), identical from run to run; --full brings the extra measurements back."""
    L = 50001
    common = ["--individuals", "1000", "--markers", str(L), "--steps", "2", "--warmup", "1"]
    lines = []
    for k in range(2):
        r = _run(common + ["--dump-outputs", str(tmp_path / str(k))], timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = lines[0]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] - L / (line["ms_per_step"] / 1e3)) <= 1e-9 * line["value"]
    assert line["cpu_baseline"] is None and line["parity"] is None
    assert not {"genotype_pass", "scan_fp64_mode", "config_C2_5000x500000"} & set(line["roofline_secondary"])
    d0, d1 = _load_dump(str(tmp_path / "0")), _load_dump(str(tmp_path / "1"))
    assert sorted(d0) == ["a", "selected_marker", "tsqmax", "vara"]
    assert all(x.dtype == np.float64 for x in d0.values()) and d0["a"].shape == d0["vara"].shape == (L,)
    assert all(np.array_equal(d0[k], d1[k]) for k in d0)
    with np.errstate(all="ignore"):
        tsq = d0["a"] ** 2 / d0["vara"]
    assert int(np.nanargmax(tsq)) + 1 == int(d0["selected_marker"][0]) == line["selected_marker"] == lines[1]["selected_marker"]
    assert d0["tsqmax"][0] == line["tsqmax"]
    r = _run(common + ["--full", "--no-secondary", "--cpu-sample", "4096"], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    full = json.loads(r.stdout.strip().splitlines()[-1])
    assert full["cpu_baseline"]["value"] > 0 and "gate" in full["parity"] and "genotype_pass" in full["roofline_secondary"]
    assert full["selected_marker"] == line["selected_marker"]


@pytest.mark.gpu
@pytest.mark.parametrize("ranks,n", [(2, 3200), (4, 3000)])
def test_rank_rehearsal_through_the_self_spawn_path(tmp_path, ranks, n):
    """Two / four ranks sharing the one card (gloo: collectives through the host), started by bench.py itself, select the marker one
    rank selects, with the same tsq; the JSON says how many ranks RCCL saw (0 here: no RCCL transfer has run on this box).  n = 3,000
    pads to 24 row tiles of 128, so four ranks SHARE the rows of W (one all-gather) when that is the faster form; 3,200 pads to 26."""
    common = ["--individuals", str(n), "--markers", "150001", "--steps", "2", "--warmup", "1", "--no-secondary", "--cpu-sample", "0"]
    one = json.loads(_run(common + ["--dump-outputs", str(tmp_path / "one")], timeout=900).stdout.strip().splitlines()[-1])
    many_p = _run(["--gpus", str(ranks)] + common + ["--dump-outputs", str(tmp_path / "many")], env={"EAGLE_BENCH_BACKEND": "gloo"}, timeout=900)
    assert many_p.returncode == 0, many_p.stderr[-2000:]
    many = json.loads(many_p.stdout.strip().splitlines()[-1])
    assert one["n_gpus"] == 1 and many["n_gpus"] == ranks
    assert many["launcher"].startswith("self-spawned") and many["rccl_ranks"] == 0 and "gloo" in many["collective_backend"]
    assert sum(many["markers_per_rank"]) == 150001 and len(many["markers_per_rank"]) == ranks
    assert max(many["markers_per_rank"]) - min(many["markers_per_rank"]) <= 1
    assert many["selected_marker"] == one["selected_marker"]
    # the rows of W come from the row-block product when they are shared between ranks: same sums in another order
    assert abs(many["tsqmax"] - one["tsqmax"]) <= 1e-9 * abs(one["tsqmax"])
    if "replicated" in many["w_sharing"]:
        assert many["tsqmax"] == one["tsqmax"]
    # the dump of N ranks is the shards' results gathered in marker order: the one-rank arrays (vara to the certified 1e-7)
    d1, dn = _load_dump(str(tmp_path / "one")), _load_dump(str(tmp_path / "many"))
    assert d1["a"].shape == dn["a"].shape == (150001,) and dn["selected_marker"][0] == many["selected_marker"]
    np.testing.assert_allclose(dn["a"], d1["a"], rtol=1e-9, atol=1e-12 * np.abs(d1["a"]).max())
    np.testing.assert_allclose(dn["vara"], d1["vara"], rtol=1e-7)
    assert one["rccl_ranks"] == 0 and one["launcher"] == "single process"
