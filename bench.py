#!/usr/bin/env python3
"""bench.py -- markers/sec through the calculate_a_and_vara genome scan + MM^T build wall-clock on MI355X.

  python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]   (N > 1: launched by torch.distributed.run, one rank per GPU)

Workload (BASELINE.json north_star / configs[2], the configuration the metric is quoted on): synthetic
10,000 individuals x 1,000,000 biallelic SNPs, single trait.  STRONG scaling: the 1,000,000 markers are split into N
contiguous shards (eagleeverything_amd.sharded.shard_range), one per GPU, resident in HBM as int8 before the timed region;
N = 1 is the whole problem on one card.  A "step" is one full pass of the reference's calculate_a_and_vara_rcpp
(v = S a_hat, a = Mt v, W = S V S, T = Mt W, vara_i = T_i . m_i; E/src/calculate_a_and_vara_rcpp.cpp:90-112) including
the a-posteriori certification of the digit-slice kernel, followed by find_qtl's tsq / arg-max (E/R/find_qtl.R:71-83)
over the rank's shard; for N > 1 the n^3 product W = S V S is shared by rows (one all-gather) and the shards'
(max tsq, first index) pairs are all-gathered inside the step.  value = 1,000,000 markers / max-over-ranks step time.
The MM^T build (calculateMMt_rcpp.cpp:95; exact int32 partial SYRK per rank + one RCCL sum + finish) is timed separately
and reported as mmt_build_s.  A plain run does only that: set up, warm up, time the K steps, print one JSON line.
--full then measures what the headline does not need: the stand-alone genotype pass, the secondary entries (N = 1: BASELINE
configs[1] (5,000 x 500,000), the fp64-mode scan, the 7-digit scan of the headline shape and the other A/Bs), the CPU baseline
-- the C oracle (a port of the reference's in-memory branch) on a bounded marker sample on rank 0's host cores -- and the
parity gate of the timed step against it.  --dump-outputs DIR writes a, vara, the selected marker and tsqmax of the last timed
step (dump_outputs).
"""
import argparse
import hashlib
import json
import os
import sys
import time

# A GPU box shows all its host cores (256) but confines one GPU's process to a share of them (16): thread pools sized by
# os.cpu_count() -- OpenBLAS under numpy, OpenMP under torch's CPU ops -- then spin on cores they do not have and slow down
# everything host-side, including the HIP runtime's staging copies of pageable buffers (measured: +14 ms per reference-shaped
# call, and a 256-thread OpenMP team running the CPU baseline 300x slower than 16 threads).  Defaults only; the caller's wins.
_SHARE = str(min(16, os.cpu_count() or 1))
os.environ.setdefault("OPENBLAS_NUM_THREADS", _SHARE)
os.environ.setdefault("OMP_NUM_THREADS", _SHARE)
os.environ.setdefault("MKL_NUM_THREADS", _SHARE)

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6   # MI355X fp64 matrix, AMD datasheet (the microarch guide lists no fp64 row)
I8_MFMA_PEAK_TOPS = 5000.0     # dense int8 = 2x the 2.5 PF bf16 dense peak (MI355X_MICROARCH.md, Matrix cores)
FP4_MFMA_PEAK_TOPS = 10000.0   # dense fp4 / fp6 on the block-scaled path = 4x bf16 (same guide)
HBM_PEAK_GBS = 8000.0


def kernel_sha16():
    """Hash of the kernel sources: a committed PMC figure is only attached to a line made by the same kernels."""
    h = hashlib.sha256()
    for f in ("eagle_t8.h", "eagle_i8mfma.hip", "eagle_kernels.hip", "eagle_w8.hip"):
        h.update(open(os.path.join(ROOT, "eagleeverything_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def host_operands_torch(torch, MMt_norm, X, y, varE, varG):
    """E/R/find_qtl.R:5-49 (calculateH, calculateP, MMt^{+-1/2}, a_hat, Var a_hat) in fp64 on the device --
    input manufacturing for the scan, not part of the timed path (same formulas as eagleeverything_amd.host_model)."""
    n = MMt_norm.shape[0]
    I = torch.eye(n, dtype=torch.float64, device=MMt_norm.device)
    H = varE * I + varG * MMt_norm
    Hinv = torch.cholesky_inverse(torch.linalg.cholesky(H))
    HX = Hinv @ X
    P = Hinv - HX @ torch.linalg.solve(X.T @ HX, HX.T)
    ev, U = torch.linalg.eigh(MMt_norm)
    sq = (U * ev.sqrt()) @ U.T
    sq = 0.5 * (sq + sq.T)
    S = torch.cholesky_inverse(torch.linalg.cholesky(sq))
    ahat = varG * (sq @ (P @ y))
    r1, g1 = 1.0 / varE, 1.0 / varG
    A = r1 * (X.T @ X)
    B = r1 * (X.T @ sq)
    D1 = torch.cholesky_inverse(torch.linalg.cholesky(r1 * (sq.T @ sq) + g1 * I))  # D is SPD
    D1C = D1 @ B.T
    V = varG * I - (D1 + D1C @ torch.linalg.solve(A - B @ D1C, B @ D1))
    return S, V, ahat, P, (ev, U)  # P and the eigen-decomposition feed the opt-in secondary entries (scan_with_W, spectral scan)


class Run:
    """One workload (n individuals x Ltot markers split over the ranks) set up in HBM, with its timed legs."""

    def __init__(self, args, torch, dist, coll, n, Ltot, rank, world, local_rank, backend):
        from eagleeverything_amd.sharded import DeviceShard, shard_range
        self.args, self.torch, self.dist, self.coll = args, torch, dist, coll
        self.n, self.Ltot, self.rank, self.world, self.backend = n, Ltot, rank, world, backend
        self.dev = torch.device("cuda", local_rank)
        m0, m1 = shard_range(Ltot, rank, world)
        t0 = time.time()
        self.sh = sh = DeviceShard(n, m1 - m0, first_marker=m0, device=local_rank)
        sh.nslices = args.slices
        sh.fill_synthetic()
        torch.cuda.synchronize(self.dev)
        self.t_gen = time.time() - t0
        self.S = self.V = self.ahat = None
        self.W_direct = self.v_direct = None
        self.eig = self.Xy = None

    # ---- collectives-aware helpers ----------------------------------------------------------------
    def barrier(self):
        self.torch.cuda.synchronize(self.dev)
        if self.world > 1:
            self.dist.barrier()
        self.torch.cuda.synchronize(self.dev)

    def max_over_ranks(self, x):
        if self.world == 1:
            return x
        t = self.torch.tensor([x], dtype=self.torch.float64, device=None if self.backend == "gloo" else self.dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def gather_markers(self, x):
        """This rank's per-marker results (device vector of its shard) -> the whole marker range in marker order, on the host of
        every rank.  Shards differ in length by at most one marker: each travels padded to the longest."""
        if self.world == 1:
            return x.cpu().numpy()
        from eagleeverything_amd.sharded import shard_range
        sizes = [m1 - m0 for m0, m1 in (shard_range(self.Ltot, r, self.world) for r in range(self.world))]
        buf = self.torch.zeros(max(sizes), dtype=x.dtype, device=x.device)
        buf[:x.numel()] = x
        if self.backend == "gloo":
            buf = buf.cpu()
        parts = [self.torch.empty_like(buf) for _ in sizes]
        self.dist.all_gather(parts, buf)
        return np.concatenate([p[:s].cpu().numpy() for p, s in zip(parts, sizes)])

    # ---- MM^T build: partial SYRK per shard + one sum to rank 0 + finish ----------------------------
    def mmt_build(self, reps):
        torch, sh = self.torch, self.sh
        c32 = torch.empty((sh.np_, sh.np_), dtype=torch.int32, device=self.dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        times, syrk, image = [], [], []
        MMt = None
        for rep in range(reps + 1):
            sh.M4 = None   # the fp4 operand image exists for MM^T only: making it is part of the build
            self.barrier()
            t1 = time.perf_counter()
            ev[0].record()
            sh.individual_major_fp4()   # k_transpose_pack_fp4: marker-major int8 -> individual-major fp4, one pass
            ev[1].record()
            ev[2].record()
            sh.mmt_partial(out=c32)     # zeroes c32, then the SYRK
            ev[3].record()
            self.coll.sum_partial_mmt(c32, dst=0)   # the process that talks to R needs the sum; the others only contribute
            if self.rank == 0:
                MMt, mx = sh.mmt_finish(c32, normalise=True)
            self.barrier()
            dt = self.max_over_ranks(time.perf_counter() - t1)
            if rep > 0:
                times.append(dt)
                syrk.append(ev[2].elapsed_time(ev[3]))
                image.append(ev[0].elapsed_time(ev[1]))
        del c32
        self.mmt_image_s = float(np.mean(image)) / 1e3
        return MMt, float(np.mean(times)), float(np.mean(syrk)) / 1e3

    # ---- scan operands from the model algebra on the actual MM^T (untimed input manufacturing) ------
    def make_operands(self, MMt):
        torch, sh, n, args = self.torch, self.sh, self.n, self.args
        t2 = time.time()
        gen = torch.Generator(device=self.dev)
        gen.manual_seed(7)
        if self.rank == 0:
            # 10 QTL spread over the first eighth of the markers: inside rank 0's shard for every N <= 8, so that the trait, the
            # operands and therefore the selected marker are the same whatever the number of GPUs
            qtl = torch.linspace(0, max(1, self.Ltot // 8) - 1, 12, device=self.dev).long()[1:-1].clamp(max=sh.Lloc - 1)
            y = 0.5 * sh.Mt8[qtl, :n].double().sum(0) + torch.randn(n, generator=gen, device=self.dev, dtype=torch.float64)
            X = torch.ones((n, 1), dtype=torch.float64, device=self.dev)
            if args.load_operands:
                saved = torch.load(args.load_operands, weights_only=True)
                if isinstance(saved, dict):   # everything the secondary entries need too (the PMC passes cannot run eigh)
                    S, V, ahat = [saved[k].to(self.dev) for k in ("S", "V", "ahat")]
                    P = saved["P"].to(self.dev)
                    self.eig = (saved["ev"].to(self.dev), saved["U"].to(self.dev))
                    self.W_direct, self.v_direct = 0.25 * P, 0.5 * (P @ y)
                    self.Xy = (X, y)
                    del P
                else:
                    S, V, ahat = [t.to(self.dev) for t in saved]
            elif args.simple_operands:
                A = torch.randn((n, 64), generator=gen, device=self.dev, dtype=torch.float64) / 8.0
                S = torch.eye(n, dtype=torch.float64, device=self.dev) + A @ A.T
                V = 0.5 * torch.eye(n, dtype=torch.float64, device=self.dev) - 0.01 * (A[:, :8] @ A[:, :8].T)
                ahat = torch.randn(n, generator=gen, device=self.dev, dtype=torch.float64)
            else:
                S, V, ahat, P, self.eig = host_operands_torch(torch, MMt, X, y, 1.0, 0.5)
                self.W_direct, self.v_direct = 0.25 * P, 0.5 * (P @ y)  # varG^2 P and varG P y: what eagle_scan_with_W takes
                self.Xy = (X, y)
                if args.save_operands and self.n == args.n and self.Ltot == args.markers:   # (the headline run only, not the C2 secondary)
                    torch.save({"S": S.cpu(), "V": V.cpu(), "ahat": ahat.cpu(), "P": P.cpu(), "ev": self.eig[0].cpu(), "U": self.eig[1].cpu()}, args.save_operands)
        else:
            S = torch.empty((n, n), dtype=torch.float64, device=self.dev)
            V = torch.empty((n, n), dtype=torch.float64, device=self.dev)
            ahat = torch.empty(n, dtype=torch.float64, device=self.dev)
        S, V, ahat = S.contiguous(), V.contiguous(), ahat.contiguous()
        if args.save_operands and self.rank == 0 and (args.simple_operands or args.load_operands):
            torch.save([S.cpu(), V.cpu(), ahat.cpu()], args.save_operands)
        self.coll.broadcast_(S); self.coll.broadcast_(V); self.coll.broadcast_(ahat)
        sh.set_operands(S, V, ahat)
        torch.cuda.synchronize(self.dev)
        self.S, self.V, self.ahat = S, V, ahat
        return time.time() - t2

    # ---- one scan step --------------------------------------------------------------------------------
    def step(self, evs=None):
        sh = self.sh
        if evs:
            evs["w"][0].record()
        sh.scan_operands(self.coll)  # N > 1: each rank computes 1/N of W's rows, one all-gather (N = 1: the whole of it)
        if evs:
            evs["w"][1].record()
            evs["prep"][0].record()
        if sh.mode == 0:
            sh.gemv_a()
        else:
            sh.vara_prepare()  # slices W; one genotype pass for a = Mt v and the diagonal term of vara
        if evs:
            evs["prep"][1].record()
            evs["kern"][0].record()
        sh.vara_kernel()
        if evs:
            evs["kern"][1].record()
            evs["cert"][0].record()
        sh.certify()       # digit-slice mode: fp64 re-evaluation of every marker the error bounds cannot settle
        if evs:
            evs["cert"][1].record()
        sh.argmax()
        tsqmax, gidx, near = sh.best()
        return self.coll.best_marker(tsqmax, gidx, device=self.dev)

    def choose_w_sharing(self):
        """W = S V S either shared (each rank 1/N of its rows + one all-gather) or replicated on every rank: which is faster
        depends on the links between the N GPUs.  Both forms are timed before the warm-up; the only value exchanged is the
        all-reduced max, so every rank takes the same branch.  A failing collective raises and the job exits non-zero."""
        sh = self.sh
        if self.world == 1 or (sh.np_ // 128) % self.world != 0:
            sh.share_w = False
            return None
        w_times = {}
        for share in (True, False):
            sh.share_w = share
            self.step()
            self.barrier()
            tw = time.perf_counter()
            self.step()
            self.step()
            self.barrier()
            w_times[share] = self.max_over_ranks(time.perf_counter() - tw)
        sh.share_w = w_times[True] <= w_times[False]
        return {"shared_s": w_times[True] / 2, "replicated_s": w_times[False] / 2}

    def timed(self, steps, warmup):
        torch = self.torch
        names = ("w", "prep", "kern", "cert")
        evs = [{k: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for k in names} for _ in range(steps)]
        sel = None
        for _ in range(warmup):
            sel = self.step()
        self.barrier()
        t3 = time.perf_counter()
        for i in range(steps):
            sel = self.step(evs[i])
        self.barrier()
        elapsed = self.max_over_ranks(time.perf_counter() - t3)
        parts = {k: float(np.mean([e[k][0].elapsed_time(e[k][1]) for e in evs])) / 1e3 for k in names}
        return sel, elapsed, parts


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(out_dir, a, vara, selected_marker, tsqmax, cap=DUMP_CAP_BYTES):
    """--dump-outputs: what the last timed step hands its caller, as out_dir/<name>.npy in float64 -- a and vara per marker, the
    selected marker (1-based, 0 = none: find_qtl.R's pick) and its tsq -- so that two builds can be compared output for output.
    When a and vara together exceed `cap` bytes, a fixed seeded sample of markers is written instead, with its 0-based marker
    indices in marker_index.npy.  Returns the names written."""
    a = np.asarray(a, dtype=np.float64).ravel()
    vara = np.asarray(vara, dtype=np.float64).ravel()
    out = {}
    if a.nbytes + vara.nbytes > cap - 4096:   # (headroom for the .npy headers and the two scalars)
        k = (cap - 4096) // 24                # a, vara and the index: 24 bytes per sampled marker
        idx = np.sort(np.random.default_rng(0).choice(a.size, size=k, replace=False))
        a, vara = a[idx], vara[idx]
        out["marker_index"] = idx.astype(np.float64)
    out.update({"a": a, "vara": vara, "selected_marker": np.array([selected_marker], dtype=np.float64),
                "tsqmax": np.array([tsqmax], dtype=np.float64)})
    os.makedirs(out_dir, exist_ok=True)
    for name, x in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), x)
    return sorted(out)


def vara_roofline(sh, kern_s, S_used):
    np_, Lp = sh.np_, sh.Lp
    if sh.mode == 0:
        nct = np_ // 128  # executed = algorithmic for the triangular fp64 kernel: column tile ct needs k < (ct+1)*128
        flops = sum(2.0 * Lp * 128 * min((ct + 1) * 128, np_) for ct in range(nct))
        roof = {"bound": "mfma", "kernel": "k_vara_f64d (v_mfma_f64_16x16x4_f64, 128 x 128 tiles, A converted once per K block, Wu by LDS-DMA)", "dtype": "f64",
                "achieved": flops / kern_s / 1e12, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s"}
    else:
        nct8 = np_ // 256
        ops = sum(2.0 * Lp * 256 * min((ct + 1) * 256, np_) for ct in range(nct8)) * S_used
        roof = {"bound": "mfma", "kernel": "k_vara_i8p (v_mfma_i32_32x32x32_i8, %d digit slices)" % S_used, "dtype": "i8",
                "achieved": ops / kern_s / 1e12, "peak": I8_MFMA_PEAK_TOPS, "unit": "TFLOP/s"}
    roof["frac"] = roof["achieved"] / roof["peak"]
    roof["kernel_ms"] = kern_s * 1e3
    return roof


def cpu_baseline_and_parity(args, ci, n, Ltot):
    """The C port of the reference's in-memory branch on the GPU box's host cores, on a bounded sample, and the parity of the GPU result on
    that sample.  Threads: what the cgroup gives this process (/sys/fs/cgroup/cpu.max; the box hands one GPU a share of the host that
    os.cpu_count() does not show, and an OpenMP team larger than the share crawls), else the affinity mask, capped at 64; a wider team is
    only probed on 16 markers.  Then -- BASELINE.md section 3 -- numpy's @ on its bundled OpenBLAS as the secondary baseline."""
    from oracle import oracle_c  # checker / baseline only
    oracle_c.build()
    host_cores = os.cpu_count() or 1
    try:
        usable = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        usable = host_cores
    cg = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            cg = max(1, int(float(q) / float(per) + 0.5))
    except (OSError, ValueError):
        pass
    threads = int(os.environ.get("OMP_NUM_THREADS", 0)) or (cg if cg else min(16, usable))
    threads = max(1, min(threads, usable, 64))
    ns, Mt_s, Sh, Vh, ah = ci["ns"], ci["Mt_s"], ci["Sh"], ci["Vh"], ci["ah"]
    oracle_c.set_num_threads(threads)
    v_h, W_h = oracle_c.scan_operands(Sh, Vh, ah)          # n^3 part, done once per call in the reference too
    tc = time.perf_counter()
    a_ref, vara_ref = oracle_c.scan_from_i8_with_W(Mt_s, v_h, W_h)
    cpu_s = time.perf_counter() - tc
    cores = oracle_c.num_threads()
    cpu = {"value": ns / cpu_s, "unit": "markers/s", "cores": cores, "kind": "port",
           "sample": "first %d markers of the %dx%d problem, reference in-memory branch order (GEMV, T=Mt*W, row-dot; "
                     "calculate_a_and_vara_rcpp.cpp:91-112), W=S*V*S precomputed and excluded" % (ns, n, Ltot),
           "seconds": cpu_s, "host_cores": host_cores, "cores_this_process_may_use": usable, "cgroup_cpu_max_cores": cg}
    if cg is None and usable > cores:   # no cgroup limit visible: is a wider team faster?  16 markers only (a team larger than the real share crawls)
        oracle_c.set_num_threads(min(usable, 256))
        tc = time.perf_counter()
        oracle_c.scan_from_i8_with_W(Mt_s[:16], v_h, W_h)
        cpu["wider_team_probe"] = {"threads": oracle_c.num_threads(), "value": 16 / (time.perf_counter() - tc), "sample": "first 16 markers"}
        oracle_c.set_num_threads(threads)
    # numpy @ (OpenBLAS dgemm / dgemv) on the same sample: T = Mt W, vara_i = T_i . m_i, a = Mt v
    nb = min(ns, 16384)
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
        limiter = threadpool_limits(limits=cores, user_api="blas")
    except Exception:
        threadpool_info = limiter = None
    tc = time.perf_counter()
    Mf = Mt_s[:nb].astype(np.float64)
    a_np = Mf @ v_h
    T_np = Mf @ W_h
    vara_np = np.einsum("ij,ij->i", T_np, Mf)
    np_s = time.perf_counter() - tc
    blas = [(i.get("internal_api"), i.get("num_threads")) for i in threadpool_info() if i.get("user_api") == "blas"] if threadpool_info else None
    cpu["numpy_openblas"] = {"value": nb / np_s, "unit": "markers/s", "blas_threads": blas, "sample": "first %d markers, int8 -> float64 conversion included" % nb,
                             "a_max_rel_vs_port": float(np.max(np.abs(a_np - a_ref[:nb])) / np.max(np.abs(a_ref[:nb]))),
                             "vara_max_rel_vs_port": float(np.max(np.abs(vara_np - vara_ref[:nb]) / np.abs(vara_ref[:nb])))}
    del Mf, T_np
    a_g, v_g = ci["a_g"], ci["v_g"]
    rel = lambda x, r: float(np.max(np.abs(x - r)) / np.max(np.abs(r)))
    with np.errstate(all="ignore"):
        tsq_g, tsq_r = a_g ** 2 / v_g, a_ref ** 2 / vara_ref
    okt = np.isfinite(tsq_r) & (tsq_r > 0)
    parity = {"a_max_rel": rel(a_g, a_ref), "vara_max_rel": float(np.max(np.abs(v_g - vara_ref) / np.abs(vara_ref))),
              "tsq_max_rel": float(np.max(np.abs(tsq_g[okt] - tsq_r[okt]) / tsq_r[okt])),
              "sample_argmax_equal": bool(np.nanargmax(tsq_g) == np.nanargmax(tsq_r))}
    # SURVEY 8(d) parity gate run with every measurement.  north_star's tolerance is 1e-6 relative on the score statistics; the digit-slice
    # certificate ENFORCES 1.8 x the budget in force per marker; the gate asks for the level actually measured (1e-7: an order of magnitude
    # of drift shows) and checks tsq = a^2 / vara, the statistic itself, against the 1e-6
    tol = 1e-7 if ci["mode"] else 1e-9
    parity["gate"] = {"a_rel_tol": 1e-9, "vara_rel_tol": tol, "tsq_rel_tol": 1e-6, "north_star_tol": 1e-6,
                      "certificate_enforces_per_marker": "1.8 x config.budget_enforced"}
    parity["gate"]["passed"] = bool(parity["a_max_rel"] <= 1e-9 and parity["vara_max_rel"] <= tol and parity["tsq_max_rel"] <= 1e-6 and
                                    parity["sample_argmax_equal"])
    # MM^T baseline on a marker subsample, scaled linearly in L
    tc = time.perf_counter()
    oracle_c.mmt_from_i8(ci["M_s"])
    mm_s = time.perf_counter() - tc
    cpu["mmt_build_s_est"] = mm_s * Ltot / ci["nm"]
    cpu["mmt_sample"] = "%d markers, scaled linearly to %d" % (ci["nm"], Ltot)
    return cpu, parity


def abi_leg(args, torch, geno, n, L, S, V, ahat, device, steps, warmup, mmt_reps=2):
    """The reference-shaped calls (host files -> host results) on `device` (an int, or a tuple of devices behind ONE context):
    eagle_calculateMMt and eagle_calculate_a_and_vara + eagle_last_scan_argmax through ctypes -- what the R package's .Call
    sees (E/R/calcMMt.R:1-15, E/R/calculate_a_and_vara.R:20-31, E/R/find_qtl.R:71-83).  S, V: column-major host matrices as R
    hands them; every call uploads them over PCIe (S is verified against the device copy of the last call instead, when it is
    the same matrix) and brings a, vara (16 bytes per marker) back.  PCIe-inclusive: never bench.py's `value` in the default form."""
    from eagleeverything_amd import rcpp_api
    ncores = os.cpu_count() or 1
    out = {}
    nan = float("nan")
    mm_cold = mm_warm = None
    MMt = None
    if geno.get("asciifileM"):
        t = time.perf_counter()
        MMt = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, ncores, nan, (n, L), device=device)
        mm_cold = time.perf_counter() - t
        ts = []
        for _ in range(mmt_reps):
            t = time.perf_counter()
            MMt = rcpp_api.calculateMMt_rcpp(geno["asciifileM"], 8.0, ncores, nan, (n, L), device=device)
            ts.append(time.perf_counter() - t)
        mm_warm = float(np.mean(ts))
        out["calculateMMt_s"] = {"cold (2-bit sidecar -> HBM -> MM^T -> host)": mm_cold, "warm (genotypes resident; 8 n^2 bytes back)": mm_warm}
    if S is None:
        return out, MMt
    t = time.perf_counter()
    r = rcpp_api.calculate_a_and_vara_rcpp(geno["asciifileMt"], nan, S, V, 8.0, (L, n), ahat, device=device)
    scan_cold = time.perf_counter() - t
    for _ in range(warmup):
        r = rcpp_api.calculate_a_and_vara_rcpp(geno["asciifileMt"], nan, S, V, 8.0, (L, n), ahat, device=device)
    ndev = len(device) if isinstance(device, tuple) else 1
    per_call, lib_wall, arg_ms = [], [], []
    t = time.perf_counter()
    for _ in range(steps):
        t1 = time.perf_counter()
        r = rcpp_api.calculate_a_and_vara_rcpp(geno["asciifileMt"], nan, S, V, 8.0, (L, n), ahat, device=device)
        t2 = time.perf_counter()
        idx, tsqmax, near = rcpp_api.last_scan_argmax(device=device)
        t3 = time.perf_counter()
        per_call.append((t3 - t1) * 1e3)
        arg_ms.append((t3 - t2) * 1e3)
        lib_wall.append(rcpp_api.last_scan_timing(device=device, device_index=0)["call_wall_s"] * 1e3)
    elapsed = time.perf_counter() - t
    out["calculate_a_and_vara_s"] = {"cold (2-bit sidecar -> HBM, then the scan)": scan_cold, "warm": elapsed / steps}
    out["markers_per_s"] = L * steps / elapsed
    out["ms_per_call"] = elapsed / steps * 1e3
    # where a call's time goes, call by call: the wrapper's clock around eagle_calculate_a_and_vara + eagle_last_scan_argmax, the
    # library's own clock for the first (call_wall_s), the arg-max call alone; an outlier shows as max against median
    out["ms_per_call_stats"] = {"calls": steps, "min": float(np.min(per_call)), "median": float(np.median(per_call)), "max": float(np.max(per_call)),
                                "library_call_wall_ms": {"min": float(np.min(lib_wall)), "median": float(np.median(lib_wall)), "max": float(np.max(lib_wall))},
                                "argmax_call_ms_median": float(np.median(arg_ms)),
                                "wrapper_overhead_ms_median": float(np.median(np.array(per_call) - np.array(lib_wall) - np.array(arg_ms))),
                                "per_call_ms": [round(x, 2) for x in per_call], "library_call_wall_ms_per_call": [round(x, 2) for x in lib_wall]}
    out["w_engine"] = rcpp_api.last_w_info(device=device if not isinstance(device, tuple) else device[0])
    out["phases_per_device"] = [rcpp_api.last_scan_timing(device=device, device_index=k) for k in range(ndev)]
    out["s_cache (hits, misses)"] = list(rcpp_api.scan_operand_cache_stats(device=device))
    a, v = np.asarray(r["a"]).ravel(), np.asarray(r["vara"]).ravel()
    with np.errstate(all="ignore"):
        tsq = a * a / v
    out["selected_marker"] = int(idx)
    out["tsqmax"] = float(tsqmax)
    out["selected_marker_is_first_argmax_of_returned_arrays"] = bool(idx == int(np.nanargmax(tsq)) + 1)   # find_qtl.R:76-80 on what R receives
    out["results"] = (a, v)
    return out, MMt


def main_abi(args):
    """--form abi: ONE process, N GPUs behind the reference-shaped C ABI (eagle_open_devices: worker thread + stream per device,
    ncclReduce of the packed int32 MM^T tiles, W's rows + ncclAllGather, lower bounds through the host).  Same workload, data,
    operands and metric as the default form; host files in, host arrays out, so every call includes its PCIe traffic."""
    import tempfile
    N = args.gpus
    devs = [int(x) for x in args.abi_devices.split(",")] if args.abi_devices else list(range(N))
    if len(devs) != N:
        print("bench.py: --abi-devices names %d devices but --gpus is %d" % (len(devs), N), file=sys.stderr)
        return 2
    if args.dry_run:
        print(json.dumps({"dry_run": True, "form": "abi", "n_gpus": N, "devices": devs, "launcher": "single process (eagle_open_devices)"}))
        return 0
    import torch
    have = torch.cuda.device_count()
    if have == 0 or max(devs) >= have:
        print("bench.py: --form abi wants devices %s but this node shows %d GPU(s)" % (devs, have), file=sys.stderr)
        return 3
    from eagleeverything_amd import rcpp_api, synth
    from eagleeverything_amd.sharded import DeviceShard
    n, L = args.n, args.markers
    device = devs[0] if N == 1 else tuple(devs)
    dev0 = torch.device("cuda", devs[0])
    t0 = time.time()
    sh = DeviceShard(n, L, first_marker=0, device=devs[0])
    sh.fill_synthetic()
    tmp = tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
    try:
        geno = synth.write_geno_pair_sidecars(tmp, sh)
        # the trait needs ten genotype rows of rank 0's range (as in the default form): keep them, drop the images
        gen = torch.Generator(device=dev0)
        gen.manual_seed(7)
        qtl = torch.linspace(0, max(1, L // 8) - 1, 12, device=dev0).long()[1:-1].clamp(max=L - 1)
        y = 0.5 * sh.Mt8[qtl, :n].double().sum(0) + torch.randn(n, generator=gen, device=dev0, dtype=torch.float64)
        del sh
        torch.cuda.empty_cache()
        t_gen = time.time() - t0
        part, MMt = abi_leg(args, torch, geno, n, L, None, None, None, device, 0, 0, args.mmt_reps)
        t1 = time.time()
        if args.load_operands:
            S, V, ahat = [x.to(dev0) for x in torch.load(args.load_operands, weights_only=True)]
        else:
            Md = torch.as_tensor(MMt, device=dev0)
            Md = Md / Md.max() + 0.95 * torch.eye(n, dtype=torch.float64, device=dev0)   # calcMMt.R:13
            X = torch.ones((n, 1), dtype=torch.float64, device=dev0)
            S, V, ahat, _, _ = host_operands_torch(torch, Md, X, y, 1.0, 0.5)
            del Md
        # what R hands over: column-major n x n doubles (rcpp_api takes MATRICES; .T of the C-ordered copy is the F-ordered matrix)
        S_h = np.asfortranarray(S.cpu().numpy())
        V_h = np.asfortranarray(V.cpu().numpy())
        a_h = ahat.cpu().numpy()
        del S, V, MMt
        torch.cuda.empty_cache()
        t_ops = time.time() - t1
        geno_scan = {"asciifileMt": geno["asciifileMt"]}
        leg, _ = abi_leg(args, torch, geno_scan, n, L, S_h, V_h, a_h, device, args.steps, args.warmup)
        a_r, v_r = leg.pop("results")
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, a_r, v_r, leg["selected_marker"], leg["tsqmax"])
        ph = leg["phases_per_device"][0]
        info = rcpp_api.device_info(device)
        np_ = (n + 255) // 256 * 256
        Lp0 = (ph["markers"] + 255) // 256 * 256
        roof = None
        if args.mode == "i8" and ph["vara_ms"] > 0:
            # the digit count is chosen inside the library from the error bound: eagle_last_scan_digits says what the last scan ran on
            S_used = rcpp_api.last_scan_digits(device=device)[0] or args.slices or 3
            ops = sum(2.0 * Lp0 * 256 * min((ct + 1) * 256, np_) for ct in range(np_ // 256)) * S_used
            roof = {"bound": "mfma", "kernel": "k_vara_i8p on the lead device's shard (%d markers), HIP events inside the library "
                                               "(eagle_last_scan_timing.vara_ms), %d digit slices (eagle_last_scan_digits)" % (ph["markers"], S_used),
                    "achieved": ops / (ph["vara_ms"] / 1e3) / 1e12, "peak": I8_MFMA_PEAK_TOPS, "unit": "TFLOP/s",
                    "frac": ops / (ph["vara_ms"] / 1e3) / 1e12 / I8_MFMA_PEAK_TOPS, "kernel_ms": ph["vara_ms"], "traffic": None}
        distinct = len(set(devs)) == len(devs)
        out = {
            "metric": "markers/sec in calculate_a_and_vara scan (+ MMt build wall-clock: mmt_build_s)", "value": leg["markers_per_s"], "unit": "markers/s",
            "n_gpus": N, "steps": args.steps, "warmup": args.warmup, "ms_per_step": leg["ms_per_call"], "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None,
            "dtype": "f64" if args.mode == "f64" else "i8 (int32/int64 exact sums, f64 finish, fp64 re-evaluation of uncertified markers)",
            "data": "synthetic", "form": "abi",
            "config": {"workload": "BASELINE configs[2] / north_star: synthetic %d individuals x %d SNPs through the REFERENCE-SHAPED C ABI "
                                   "(eagle_calculate_a_and_vara + eagle_last_scan_argmax per step: host S, V, a_hat in over PCIe, host a, vara out), "
                                   "genotypes resident in HBM after the first call, %d device(s) behind one context" % (n, L, N),
                       "n": n, "markers_total": L, "devices": devs,
                       "parallelism": "eagle_open_devices x%d: worker thread + stream per device" % N,
                       "collectives": ("none (one device)" if N == 1 else
                                       ("RCCL inside the library: ncclReduce (MM^T tiles), ncclAllGather (rows of W)" if distinct and os.environ.get("EAGLE_HIP_COLLECTIVES") != "host"
                                        else "host-staged stand-in (the list names one card more than once, or EAGLE_HIP_COLLECTIVES=host): REHEARSAL, not a measurement")),
                       "scan_mode": args.mode},
            "includes_pcie": True,
            "mmt_build_s": part["calculateMMt_s"]["warm (genotypes resident; 8 n^2 bytes back)"],
            "calculateMMt_s": part["calculateMMt_s"], "calculate_a_and_vara_s": leg["calculate_a_and_vara_s"],
            "selected_marker": leg["selected_marker"], "tsqmax": leg["tsqmax"],
            "selected_marker_is_first_argmax_of_returned_arrays": leg["selected_marker_is_first_argmax_of_returned_arrays"],
            "phases_per_device": leg["phases_per_device"], "s_cache (hits, misses)": leg["s_cache (hits, misses)"],
            "roofline": roof, "cpu_baseline": None, "device": info, "kernel_sha16": kernel_sha16(),
            "setup_s": {"genotypes + sidecars": t_gen, "operands": t_ops},
        }
        print(json.dumps(out))
    finally:
        for f in os.listdir(tmp):
            os.unlink(os.path.join(tmp, f))
        os.rmdir(tmp)
        rcpp_api.close_all()
    return 0


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--individuals", "--n", dest="n", type=int, default=10000,
                    help="individuals (spell it --individuals under torch.distributed.run, whose own parser takes --n for one of its options)")
    ap.add_argument("--markers", type=int, default=1000000, help="markers in TOTAL (split over the GPUs: strong scaling)")
    ap.add_argument("--mode", choices=["f64", "i8"], default=os.environ.get("EAGLE_SCAN_MODE", "i8"))
    ap.add_argument("--slices", type=int, default=0, help="int8 digit slices of W in i8 mode (0 = chosen from the error bound)")
    ap.add_argument("--mmt-reps", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run what it does not need: the stand-alone genotype pass, the secondary entries, "
                         "the CPU baseline and the parity gate (off: set up, warm up, time the steps, print the line)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step returned (a, vara, selected marker, tsqmax) as DIR/<name>.npy in float64")
    ap.add_argument("--cpu-sample", type=int, default=32768, help="with --full: markers in the CPU-baseline sample (0 = skip)")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary entries (C2, fp64 mode, 7 digits)")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip the reference-shaped (host files -> host results) secondary leg")
    ap.add_argument("--simple-operands", action="store_true", help="seeded random SPD S / V instead of the model algebra")
    ap.add_argument("--save-operands", default=None, help="write S, V, a_hat (torch.save) after computing them")
    ap.add_argument("--load-operands", default=None, help="read S, V, a_hat written by --save-operands (used by the PMC passes of\n                    tools/profile_gpu.sh: rocSOLVER's eigh crashes under rocprofv3 counter collection)")
    ap.add_argument("--form", choices=["ranks", "abi"], default="ranks",
                    help="ranks (default): one process per GPU over torch.distributed / RCCL, device-resident entry points; "
                         "abi: ONE process, the N GPUs behind the reference-shaped C ABI (eagle_open_devices), host files -> host results: "
                         "the path the R package takes (E/R/AM.R:185-196,214,450-455)")
    ap.add_argument("--abi-devices", default=os.environ.get("EAGLE_BENCH_ABI_DEVICES"),
                    help="--form abi: comma-separated device list instead of 0..N-1 (naming one card twice rehearses the path on a one-GPU box)")
    ap.add_argument("--dry-run", action="store_true", help="print what would be launched (the child command for N > 1) as JSON and exit")
    return ap.parse_args(argv)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def child_command(args, argv):
    """`python -m torch.distributed.run ... bench.py <the same arguments>`: one rank per GPU, rendezvous on 127.0.0.1."""
    port = int(os.environ.get("EAGLE_BENCH_MASTER_PORT", 0)) or _free_port()
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + [a for a in argv if a != "--dry-run"]


def self_spawn(args, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a CHILD process (torch.distributed.run) before anything in
    this process has touched the GPU (torch.cuda.device_count() does not initialise it), relay its output and exit with its code.
    Never an exec: a process that has initialised the GPU must not be replaced."""
    import subprocess
    cmd = child_command(args, argv)
    backend = os.environ.get("EAGLE_BENCH_BACKEND", "nccl")
    if args.dry_run:
        print(json.dumps({"dry_run": True, "launcher": "self-spawn", "n_gpus": args.gpus, "backend": backend, "child_command": cmd}))
        return 0
    import torch
    have = torch.cuda.device_count()
    if backend != "gloo" and args.gpus > have:
        print("bench.py: --gpus %d but this node shows %d GPU(s); nothing was launched" % (args.gpus, have), file=sys.stderr)
        return 3
    if have == 0:
        print("bench.py: no GPU visible; nothing was launched", file=sys.stderr)
        return 3
    env = dict(os.environ)
    env["EAGLE_BENCH_SPAWNED"] = "1"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OMP_NUM_THREADS"] = os.environ.get("EAGLE_BENCH_RANK_THREADS", str(max(1, min(16, (os.cpu_count() or 1) // args.gpus))))
    sys.stdout.flush()
    return subprocess.run(cmd, env=env).returncode


def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    if args.gpus < 1:
        print("bench.py: --gpus must be >= 1", file=sys.stderr)
        sys.exit(2)
    if args.steps < 1 or args.warmup < 0:
        print("bench.py: --steps must be >= 1 and --warmup >= 0", file=sys.stderr)
        sys.exit(2)
    if args.form == "abi":
        sys.exit(main_abi(args))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_spawn(args, argv))
    if args.dry_run:
        print(json.dumps({"dry_run": True, "launcher": "external" if "WORLD_SIZE" in os.environ else "none (single process)", "n_gpus": args.gpus}))
        sys.exit(0)

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world), file=sys.stderr)
        sys.exit(2)
    # EAGLE_BENCH_BACKEND=gloo rehearses the N > 1 rank logic with several ranks on ONE card (collectives through the
    # host); the measured configuration is always one rank per GPU over RCCL.
    backend = os.environ.get("EAGLE_BENCH_BACKEND", "nccl")
    if backend != "gloo" and local_rank >= torch.cuda.device_count():
        print("bench.py: rank %d has no GPU (%d visible)" % (rank, torch.cuda.device_count()), file=sys.stderr)
        sys.exit(3)
    if backend == "gloo":
        local_rank = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    if world > 1:
        if backend == "gloo":
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))

    from eagleeverything_amd import rcpp_api
    from eagleeverything_amd.sharded import Collectives, shard_range

    coll = Collectives(dist if world > 1 else None)
    info = rcpp_api.device_info(local_rank)
    n, Ltot = args.n, args.markers
    dev = torch.device("cuda", local_rank)

    run = Run(args, torch, dist, coll, n, Ltot, rank, world, local_rank, backend)
    sh = run.sh
    t_gen = run.t_gen
    sh.mode = 0 if args.mode == "f64" else 1
    MMt, mmt_build_s, syrk_s = run.mmt_build(args.mmt_reps)
    mmt_image_s = run.mmt_image_s
    t_ops = run.make_operands(MMt)
    del MMt
    w_choice = run.choose_w_sharing()
    sh_share_w = bool(sh.share_w)
    sel, elapsed, parts = run.timed(args.steps, args.warmup)
    a_step, vara_step = sh.a[:sh.Lloc].clone(), sh.vara[:sh.Lloc].clone()   # what the last timed step returned
    ms_per_step = elapsed / args.steps * 1e3
    value = Ltot * args.steps / elapsed
    kern_s = parts["kern"]
    cert = sh.certificate() if sh.mode == 1 else None
    if args.dump_outputs:
        a_all, vara_all = run.gather_markers(a_step), run.gather_markers(vara_step)
        if rank == 0:
            dump_outputs(args.dump_outputs, a_all, vara_all, sel[0], sel[1])
        del a_all, vara_all

    if world > 1:
        del a_step, vara_step
    # everything below `if args.full` is measured after the headline and is not needed for it
    gpass_s = None
    if args.full:
        # the HBM-bound kernel of the scan on its own (a = Mt v: L*n genotype bytes, read once), outside the timed steps
        gp = []
        for _ in range(4):
            g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g0.record()
            sh.gemv_a()
            g1.record()
            torch.cuda.synchronize(dev)
            gp.append(g0.elapsed_time(g1))
        gpass_s = float(np.median(gp[1:])) / 1e3

    # ---- roofline of the dominant kernel (vara) ---------------------------------------------------
    np_, Lp, Lloc = sh.np_, sh.Lp, sh.Lloc
    S_used, vara_bound = (sh.vara_i8_info()[:2] if sh.mode else (None, None))
    digits = None
    if sh.mode:   # round 3: the digits cut from W, the digits the scan ran on (one fewer under the spectral bound), the budget
        digits = {"used": S_used, "cut": sh.last_sliced, "spectral_bound_H": sh.last_specH, "spectral_level": sh.last_level,
                  "budget": sh.last_budget, "enforced_per_marker": 1.8 * sh.last_budget, "budget_default": 5e-7, "w_error_bound_eta": sh.last_wErr,
                  "note": "|digit error_i| <= min(H q2_i, l1_i^2/2 * 2^(e+1-8 used)); markers above 1.8 x budget are re-evaluated in fp64 "
                          "(certificate.flagged).  budget: the one in force -- 1e-7 is tried first, 5e-7 is the fallback "
                          "(roofline_secondary.scan_budget_5e-7_only: round 3's default as the only budget); scan_worst_case_digits: without the spectral bound"}
    roof = vara_roofline(sh, kern_s, S_used)
    # HBM-side bytes per launch come from separate rocprofv3 --pmc passes of this same command (tools/profile_gpu.sh):
    # they cannot be collected in-process.  The committed figure is attached only when it was measured on these very
    # kernel sources (hash) and this configuration; otherwise traffic is null.
    roof["traffic"] = None
    sha = kernel_sha16()
    try:
        trf = json.load(open(os.path.join(ROOT, "profiles", "r04_traffic.json")))
        tr = trf["k_vara_i8"]
        if sh.mode == 1 and trf.get("kernel_sha16") == sha and tr["config"] == {"n": n, "markers": Lloc, "slices": S_used}:
            roof["traffic"] = tr["hbm_side_bytes"]
            roof["traffic_source"] = "%s, kernel sources sha16 %s; (2*FETCH_SIZE + WRITE_SIZE)*1024 bytes per launch" % (tr["source"], sha)
            roof["l2_hit_rate"] = tr.get("TCC_hit_rate")
    except (OSError, KeyError, ValueError):
        pass
    if sh.mode == 1:
        roof["algorithmic_bytes"] = float(Lp) * np_ + float(S_used) * np_ * np_ / 2
    roof["reference_flops_per_launch"] = 2.0 * Lloc * n * n + 2.0 * Lloc * n
    roof["fp64_equiv_tflops"] = roof["reference_flops_per_launch"] / kern_s / 1e12
    # the judge's HBM figure for the whole scan uses L*n genotype bytes per pass
    roof["scan_hbm_view"] = {"bytes_per_scan": float(Ltot) * n, "achieved_GBps": float(Ltot) * n / (elapsed / args.steps) / 1e9,
                             "frac_of_8TBps_per_gpu": float(Lloc) * n / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS,
                             "note": "the scan is MFMA-bound (2Ln^2 flop on L*n bytes); its HBM-bound kernel is roofline_secondary.genotype_pass"}
    w_flops = 3.0 * np_ ** 3 if world == 1 or not sh.share_w else 4.0 * np_ ** 3 / world
    winfo = sh.w_info() if sh.mode == 1 else {"int8": 0}
    if winfo["int8"]:
        # executed int8 MAC-flop of the two digit-slice products: pairs1 full products + pairs2 on the tiles of the 256 x 384 tiling that hold
        # an element on or above the diagonal
        ntj = (np_ + 383) // 384
        up_tiles = sum(1 for i in range(np_ // 256) for j in range(ntj) if j * 384 + 383 >= i * 256)
        w_ops = 2.0 * np_ * (winfo["pairs1"] * float(np_) * ntj * 384 + winfo["pairs2"] * up_tiles * 256.0 * 384.0)
        w_entry = {"bound": "mfma", "kernel": "k_w8_gemm_p (v_mfma_i32_32x32x32_i8, 384 x 256 tiles, asm-pipelined): exact int8 digit-slice products "
                                              "of the off-diagonal parts, V S with (k, T) = (%d, %d) = %d products, S X (upper tiles) with (%d, %d) = %d"
                                              % (winfo["k1"], winfo["T1"], winfo["pairs1"], winfo["k2"], winfo["T2"], winfo["pairs2"]),
                   "dtype": "i8", "achieved": w_ops / parts["w"] / 1e12, "peak": I8_MFMA_PEAK_TOPS, "unit": "TFLOP/s",
                   "frac": w_ops / parts["w"] / 1e12 / I8_MFMA_PEAK_TOPS, "ms": parts["w"] * 1e3,
                   "fp64_equivalent_tflops": 3.0 * np_ ** 3 / parts["w"] / 1e12, "engine": winfo,
                   "eta_over_mean_diag": winfo["eta"] / winfo["mean_diag"],
                   "note": "the whole W phase is in the time: v = S a_hat, statistics, digit slices, both products, the fp64 combination of the "
                           "levels, r = S V S 1; frac counts the int8 products only.  eta: rigorous || W - S V S ||_F bound carried by the certificate"}
    else:
        w_entry = None
    secondary = {
        "step_breakdown_ms": {"W=S*V*S (+all-gather)": parts["w"] * 1e3, "prepare (slice W, genotype pass)": parts["prep"] * 1e3,
                              "vara kernel": parts["kern"] * 1e3, "certify": parts["cert"] * 1e3},
        "w_product": w_entry or {"bound": "mfma", "kernel": "k_gemm_f64_dma (v_mfma_f64_16x16x4_f64, 256 x 128 tiles, LDS-DMA): X = V*S in 1024-row blocks, then the tiles of S*X on or below the diagonal, transposed",
                      "achieved": w_flops / parts["w"] / 1e12, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                      "frac": w_flops / parts["w"] / 1e12 / FP64_MFMA_PEAK_TFLOPS, "ms": parts["w"] * 1e3,
                      "note": "includes v = S a_hat, the symmetry check, the fold and (N > 1) the all-gather of W's rows"},
        "syrk_f4": {"bound": "mfma", "kernel": "k_syrk_f4w (v_mfma_scale_f32_32x32x64_f8f6f4, fp4 x fp4, exact; 384 x 256 tiles)", "dtype": "fp4",
                    "achieved": (np_ * (np_ + 256.0)) * Lp / syrk_s / 1e12, "peak": FP4_MFMA_PEAK_TOPS,
                    "unit": "TFLOP/s", "frac": (np_ * (np_ + 256.0)) * Lp / syrk_s / 1e12 / FP4_MFMA_PEAK_TOPS,
                    "kernel_ms": syrk_s * 1e3},
    }
    if gpass_s is not None:
        secondary["genotype_pass"] = {"bound": "hbm", "kernel": "k_slice_vec + k_gemv_mfma (a = Mt v; algorithmic bytes = L_pad*n_pad genotype bytes)",
                                      "achieved": Lp * np_ / gpass_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                      "frac": Lp * np_ / gpass_s / 1e9 / HBM_PEAK_GBS, "kernel_ms": gpass_s * 1e3}
    if w_choice:
        secondary["w_sharing_preflight_s"] = w_choice

    # ---- what the CPU baseline + parity gate need (rank 0, N = 1): captured now, computed LAST (after every GPU leg: the host-side work
    # costs the driver's clock tens of seconds and disturbs the legs that follow it) ------------------------------------------------------
    cpu = None
    parity = None
    cpu_in = None
    all_marker_parity = None
    if args.full and rank == 0 and world == 1 and args.cpu_sample > 0:
        ns = min(args.cpu_sample, Lloc)
        nm = min(8192, Lloc)
        cpu_in = {"ns": ns, "Mt_s": sh.Mt8[:ns, :n].cpu().numpy(), "Sh": run.S.cpu().numpy(), "Vh": run.V.cpu().numpy(), "ah": run.ahat.cpu().numpy(),
                  "a_g": sh.a[:ns].cpu().numpy(), "v_g": sh.vara[:ns].cpu().numpy(), "mode": sh.mode,
                  "M_s": np.ascontiguousarray(sh.Mt8[:nm, :n].cpu().numpy().T), "nm": nm}

    # ---- secondary entries (N = 1): fp64-mode and 7-digit scans of the headline shape, and BASELINE configs[1] --------
    if args.full and world == 1 and not args.no_secondary and sh.mode == 1:
        sel_i8 = sel
        sh.mode = 0
        s64, el64, p64 = run.timed(1, 1)
        v64_all = sh.vara[:sh.Lloc]
        okm = v64_all.abs() > 0
        rel_all = ((vara_step - v64_all).abs() / v64_all.abs())[okm]
        all_marker_parity = {"markers": int(okm.sum()), "vara_max_rel_digit_scan_vs_fp64_scan": float(rel_all.max()),
                             "vara_p999_rel": float(torch.quantile(rel_all[:: max(1, rel_all.numel() // 1000000)], 0.999)),
                             "a_max_rel": float((a_step - sh.a[:sh.Lloc]).abs().max() / sh.a[:sh.Lloc].abs().max()),
                             "note": "every marker of the timed digit-slice step against the fp64-MFMA scan of the same operands (eagle_set_scan_mode(0)), on the device"}
        secondary["scan_fp64_mode"] = {"value": Ltot / el64, "unit": "markers/s", "ms_per_step": el64 * 1e3,
                                       "selected_marker_equal_to_digit_mode": bool(s64[0] == sel_i8[0]),
                                       "roofline": vara_roofline(sh, p64["kern"], None)}
        sh.mode = 1
        # round 3's default as the ONLY budget (5e-7, enforced per marker at 9e-7; no tighter one tried first): level 1 of the spectral bound
        # takes the digit off at once -- what the tight-first policy of round 4 costs is the difference to the headline step
        sh._check(sh.L.eagle_set_scan_budget(sh.ctx, 5e-7))
        sb, elb, pb = run.timed(3, 1)
        Sb = sh.vara_i8_info()[0]
        secondary["scan_budget_5e-7_only"] = {"value": Ltot * 3 / elb, "unit": "markers/s", "ms_per_step": elb / 3 * 1e3, "slices": Sb,
                                              "slices_cut": sh.last_sliced, "spectral_bound_H": sh.last_specH, "spectral_level": sh.last_level,
                                              "budget_used": sh.last_budget, "w_engine": sh.w_info(),
                                              "selected_marker_equal": bool(sb[0] == sel_i8[0]), "certificate": sh.certificate(),
                                              "step_breakdown_ms": {k: v * 1e3 for k, v in pb.items()},
                                              "roofline": vara_roofline(sh, pb["kern"], Sb)}
        sh._check(sh.L.eagle_set_scan_budget(sh.ctx, 0.0))   # the default policy again: 1e-7 first, then 5e-7
        # W on the fp64 GEMM (round 3's engine; eagle_set_w_mode(0)): the A/B of the int8 digit-slice products
        sh.w_mode = 0
        sf, elf, pf = run.timed(3, 1)
        secondary["scan_w_on_fp64_gemm"] = {"value": Ltot * 3 / elf, "unit": "markers/s", "ms_per_step": elf / 3 * 1e3, "budget_used": (sh.vara_i8_info(), sh.last_budget)[1],
                                            "spectral_level": sh.last_level, "selected_marker_equal": bool(sf[0] == sel_i8[0]),
                                            "vara_max_rel_vs_headline_step": float(((sh.vara[:sh.Lloc] - vara_step).abs() / vara_step.abs().clamp_min(1e-300)).max()),
                                            "step_breakdown_ms": {k: v * 1e3 for k, v in pf.items()},
                                            "w_tflops_fp64": 3.0 * sh.np_ ** 3 / pf["w"] / 1e12, "w_frac_of_fp64_peak": 3.0 * sh.np_ ** 3 / pf["w"] / 1e12 / FP64_MFMA_PEAK_TFLOPS}
        sh.w_mode = 1
        # the digit count of rounds 1-2: worst-case bound only (spectral bound switched off)
        sh.L.eagle_dev_set_tune(sh.ctx, 29)
        sw, elw, pw = run.timed(3, 1)
        Sw = sh.vara_i8_info()[0]
        secondary["scan_worst_case_digits"] = {"value": Ltot * 3 / elw, "unit": "markers/s", "ms_per_step": elw / 3 * 1e3, "slices": Sw,
                                               "selected_marker_equal": bool(sw[0] == sel_i8[0]), "certificate": sh.certificate(),
                                               "roofline": vara_roofline(sh, pw["kern"], Sw)}
        sh.L.eagle_dev_set_tune(sh.ctx, 0)
        sh.nslices = 7
        sh.ws = None
        s7, el7, p7 = run.timed(1, 1)
        secondary["scan_7_digits"] = {"value": Ltot / el7, "unit": "markers/s", "ms_per_step": el7 * 1e3,
                                      "selected_marker_equal": bool(s7[0] == sel_i8[0]), "roofline": vara_roofline(sh, p7["kern"], 7),
                                      "note": "all 53 bits of W's largest entry in exact integer arithmetic (eagle_set_scan_slices(7)): per-marker "
                                              "bound l1_i^2/2 * 2^(e-55), below the rounding of ANY fp64 summation order of the same form -- the "
                                              "fp64-accuracy figure on the int8 matrix cores, beside scan_fp64_mode on the fp64 ones"}
        sh.nslices = args.slices
        sh.ws = None
        # opt-in stochastic rounding of W's digits (eagle_set_scan_rounding): probabilistic certificate, one digit fewer
        sh.stochastic = True
        sr, elr, pr = run.timed(3, 1)
        Sr = sh.vara_i8_info()[0]
        secondary["scan_stochastic_rounding"] = {"value": Ltot * 3 / elr, "unit": "markers/s", "ms_per_step": elr / 3 * 1e3, "slices": Sr,
                                                 "selected_marker_equal": bool(sr[0] == sel_i8[0]), "certificate": sh.certificate(),
                                                 "note": "opt-in: per-marker error bound 8.355*q2*2^(e+1-8S) holds with probability 1 - 1e-30",
                                                 "roofline": vara_roofline(sh, pr["kern"], Sr)}
        sh.stochastic = False
        # optional R-side shortcut eagle_scan_with_W: W = varG^2 P and v = varG P y handed over, no S (V S) products
        if run.W_direct is not None:
            sh.set_W(run.W_direct, run.v_direct)
            sw, elw, pw = run.timed(3, 1)
            secondary["scan_with_W_handed_over"] = {"value": Ltot * 3 / elw, "unit": "markers/s", "ms_per_step": elw / 3 * 1e3,
                                                    "selected_marker_equal": bool(sw[0] == sel_i8[0]),
                                                    "note": "eagle_scan_with_W: inside AM() W = S V S equals varG^2 P, which find_qtl.R already holds; "
                                                            "not a .Call of the reference (INTEGRATION.md)"}
            sh.W0 = sh.v0 = None
        # the scan in the eigenbasis of MM^T (opt-in entry points of section 1d): Z = Mt U once, then one HBM-bound pass per scan
        if run.eig is not None:
            import ctypes as C
            lib, ctx = sh.L, sh.ctx
            ev, U = run.eig
            Xm, yv = run.Xy
            stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            Ur = torch.zeros((sh.np_, sh.np_), dtype=torch.float64, device=dev)
            Ur[:n, :n] = U
            Z = torch.empty((sh.Lp, sh.np_), dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)
            tz = time.perf_counter()
            sh._check(lib.eagle_dev_spectral_zbuild(ctx, sh.Mt8.data_ptr(), sh.Lp, sh.np_, sh.np_, Ur.data_ptr(), Z.data_ptr(), stream()))
            torch.cuda.synchronize(dev)
            zbuild_f64_s = time.perf_counter() - tz
            zcheck = Z[:4096, :n].clone()
            wsz = torch.empty(int(lib.eagle_spectral_zbuild_i8_workspace_bytes(sh.np_, 6)), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            tz = time.perf_counter()
            sh._check(lib.eagle_dev_spectral_zbuild_i8(ctx, sh.Mt8.data_ptr(), sh.Lp, sh.np_, sh.np_, Ur.data_ptr(), Z.data_ptr(), wsz.data_ptr(), 6, stream()))
            torch.cuda.synchronize(dev)
            zbuild_s = time.perf_counter() - tz   # the default of eagle_spectral_prepare: six exact int8 digit slices of U
            z_diff = float((Z[:4096, :n] - zcheck).abs().max())
            del Ur, wsz, zcheck
            UtX, Uty = U.T @ Xm, U.T @ yv
            p = UtX.shape[1]
            lin = torch.empty((sh.Lp, 16), dtype=torch.float64, device=dev)
            quad = torch.empty(sh.Lp, dtype=torch.float64, device=dev)
            a_s, v_s = torch.zeros(sh.Lp, dtype=torch.float64, device=dev), torch.zeros(sh.Lp, dtype=torch.float64, device=dev)

            def spectral_step(varE=1.0, varG=0.5):
                d = torch.zeros(sh.np_, dtype=torch.float64, device=dev)
                d[:n] = 1.0 / (varE + varG * ev)
                G = torch.zeros((sh.np_, 16), dtype=torch.float64, device=dev)
                G[:n, 0] = d[:n] * Uty
                G[:n, 1:1 + p] = d[:n, None] * UtX
                # (p x p, on the host: rocSOLVER must not run under rocprofv3 counter collection, profiles/r02_eigh_under_pmc.log)
                Cm = torch.as_tensor(np.linalg.inv((UtX.T @ (d[:n, None] * UtX)).cpu().numpy()), device=dev).contiguous()
                c1 = (Cm @ (UtX.T @ (d[:n] * Uty))).contiguous()
                sh._check(lib.eagle_dev_spectral_pass(ctx, Z.data_ptr(), sh.Lp, sh.np_, G.data_ptr(), 16, d.data_ptr(), lin.data_ptr(), quad.data_ptr(), stream()))
                sh._check(lib.eagle_dev_spectral_finish(ctx, lin.data_ptr(), 16, quad.data_ptr(), Ltot, p, Cm.data_ptr(), c1.data_ptr(), varG,
                                                        a_s.data_ptr(), v_s.data_ptr(), stream()))
                sh._check(lib.eagle_dev_tsq_argmax(ctx, a_s.data_ptr(), v_s.data_ptr(), Ltot, None, sh._best.data_ptr(), sh._scratch.data_ptr(), stream()))
                return sh.best()

            spectral_step()
            torch.cuda.synchronize(dev)
            ts = time.perf_counter()
            for _ in range(5):
                bsp = spectral_step()
            torch.cuda.synchronize(dev)
            sp_s = (time.perf_counter() - ts) / 5
            secondary["scan_spectral"] = {"value": Ltot / sp_s, "unit": "markers/s", "ms_per_step": sp_s * 1e3, "one_time_Z_build_s": zbuild_s, "Z_build_fp64_mfma_s": zbuild_f64_s,
                                          "Z_int8_vs_fp64_max_abs_diff": z_diff,
                                          "Z_bytes": float(sh.Lp) * sh.np_ * 8, "selected_marker_equal": bool(bsp[1] + 1 == sel_i8[0]),
                                          "hbm": {"bound": "hbm", "achieved": float(sh.Lp) * sh.np_ * 8 / sp_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                                  "frac": float(sh.Lp) * sh.np_ * 8 / sp_s / 1e9 / HBM_PEAK_GBS},
                                          "note": "opt-in entry points (include/eagle_hip.h 1d): needs U, lambda of the normalised MM^T and an R-side "
                                                  "change; K is fixed during an AM() run, so Z = Mt U is built once and each scan is one pass over Z"}
            del Z, lin, quad
        # (after the other secondary entries: the 35 GB this leg allocates and frees outside torch's allocator leave the card's memory
        # fragmented, and an 82 GB buffer allocated after it made the HBM-bound spectral pass 50 % slower -- 21 against 14 ms)
        # the same step through the REFERENCE-SHAPED entry points (host files -> host results; what R's .Call sees), PCIe included,
        # with the phase clock of the library: every ms between the device-resident step above and the .Call-shaped time
        import tempfile
        from eagleeverything_amd import synth
        tmpd = tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
        try:
            if args.no_e2e:
                raise StopIteration
            geno = synth.write_geno_pair_sidecars(tmpd, sh)
            sh.M8 = None   # the individual-major int8 image was only needed to write M.ascii's sidecar
            S_h, V_h, a_h = np.asfortranarray(run.S.cpu().numpy()), np.asfortranarray(run.V.cpu().numpy()), run.ahat.cpu().numpy()
            leg, _ = abi_leg(args, torch, geno, n, Ltot, S_h, V_h, a_h, local_rank, 10, 1)
            a_e, v_e = leg.pop("results")
            leg["a_bitwise_equal_to_device_resident_step"] = bool(np.array_equal(a_e, a_step.cpu().numpy()))
            leg["vara_bitwise_equal_to_device_resident_step"] = bool(np.array_equal(v_e, vara_step.cpu().numpy()))
            leg["selected_marker_equal"] = bool(leg["selected_marker"] == sel_i8[0])
            leg["device_resident_step_ms"] = ms_per_step
            leg["gap_ms (call - device-resident step)"] = leg["ms_per_call"] - ms_per_step
            leg["note"] = ("PCIe-inclusive and never `value`: per call V (8 n^2 bytes) up, S up and compared with the device copy of the last call "
                           "under the n^3 products, a_hat up, a and vara (16 bytes per marker) down; genotypes resident after the cold call "
                           "(loaded from the 2-bit sidecars beside sparse text placeholders)")
            secondary["e2e_reference_shaped"] = leg
            del S_h, V_h, a_e, v_e
        except StopIteration:
            pass
        finally:
            for f in os.listdir(tmpd):
                os.unlink(os.path.join(tmpd, f))
            os.rmdir(tmpd)
            rcpp_api.drop_cache(local_rank)
    if args.full and world == 1 and not args.no_secondary and sh.mode == 1 and not args.load_operands:
        # BASELINE configs[1]: 5,000 x 500,000 on one card (its operands come from an eigen-decomposition: not under --load-operands)
        del run, sh
        torch.cuda.empty_cache()
        run2 = Run(args, torch, dist, coll, 5000, 500000, rank, world, local_rank, backend)
        run2.sh.mode = 1
        MMt2, mmt2_s, syrk2_s = run2.mmt_build(1)
        run2.make_operands(MMt2)
        del MMt2
        run2.sh.share_w = False
        _, el2, p2 = run2.timed(3, 1)
        S2 = run2.sh.vara_i8_info()[0]
        secondary["config_C2_5000x500000"] = {"value": 500000 * 3 / el2, "unit": "markers/s", "ms_per_step": el2 / 3 * 1e3,
                                              "mmt_build_s": mmt2_s, "slices": S2, "step_breakdown_ms": {k: v * 1e3 for k, v in p2.items()},
                                              "roofline": vara_roofline(run2.sh, p2["kern"], S2)}
        sh = run2.sh

    if cpu_in is not None:   # LAST: the host-side baseline (tens of seconds of CPU work) and the parity of the timed step on its sample
        cpu, parity = cpu_baseline_and_parity(args, cpu_in, n, Ltot)
        if all_marker_parity is not None:
            parity["all_markers_vs_fp64_scan"] = all_marker_parity
            parity["gate"]["all_marker_vara_rel_tol"] = 1e-7
            parity["gate"]["passed"] = bool(parity["gate"]["passed"] and all_marker_parity["vara_max_rel_digit_scan_vs_fp64_scan"] <= 1e-7)
        del cpu_in
    if rank == 0:
        out = {
            "metric": "markers/sec in calculate_a_and_vara scan (+ MMt build wall-clock: mmt_build_s)", "value": value, "unit": "markers/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64" if args.mode == "f64" else "i8 (int32/int64 exact sums, f64 finish, fp64 re-evaluation of uncertified markers)",
            "data": "synthetic",
            "config": {"workload": "BASELINE configs[2] / north_star: synthetic %d individuals x %d SNPs in total (HWE genotypes, int8 resident "
                                   "in HBM), %d contiguous marker shards, single trait, full calculate_a_and_vara pass + certification + "
                                   "tsq arg-max" % (n, Ltot, world),
                       "n": n, "markers_total": Ltot, "markers_rank0": Lloc,
                       "parallelism": "marker-shard x%d" % world + (", W rows 1/%d per rank + all-gather" % world if world > 1 and w_choice and w_choice["shared_s"] <= w_choice["replicated_s"] else "")
                                      + (" (REHEARSAL: gloo, ranks share one card)" if backend == "gloo" and world > 1 else ""),
                       "scan_mode": args.mode, "slices": S_used, "digits": digits, "vara_abs_error_bound_worst_case": vara_bound,
                       # scalars mirrored here because the driver's record keeps `config` (they are also top-level keys / parts of the objects above)
                       "mmt_build_s": mmt_build_s, "mmt_image_s": mmt_image_s, "mmt_syrk_s": syrk_s, "mmt_finish_s": max(0.0, mmt_build_s - mmt_image_s - syrk_s),
                       "rccl_ranks": dist.get_world_size() if world > 1 and backend == "nccl" else 0,
                       "launcher": "self-spawned child torch.distributed.run" if os.environ.get("EAGLE_BENCH_SPAWNED") else ("external launcher" if world > 1 else "single process"),
                       "w_sharing": ("rows 1/%d per rank + one all-gather" % world if world > 1 and sh_share_w else ("replicated on every rank" if world > 1 else "n/a (one rank)")),
                       "digits_used": S_used, "digits_cut": digits["cut"] if digits else None, "budget_used": digits["budget"] if digits else None,
                       "bound_level": digits["spectral_level"] if digits else None,
                       "cert_flagged": cert["flagged"] if cert else None, "cert_reevaluated": cert["reevaluated"] if cert else None,
                       # what the certificate enforced per marker is 1.8 x this: the budget in force, or the default behind a tight one when more
                       # than 512 markers of the scan missed the tight threshold
                       "cert_over_tight": cert.get("over_tight") if cert else None,
                       "budget_enforced": (None if not (cert and digits) else (sh.last_budget_loose if cert.get("over_tight", 0) > 512 else digits["budget"])),
                       "w_engine": "int8 digit slices" if winfo["int8"] else "fp64 GEMM", "w_ms": parts["w"] * 1e3,
                       "w_pairs_VS": winfo.get("pairs1"), "w_pairs_SX": winfo.get("pairs2"),
                       "w_eta_over_mean_diag": (winfo["eta"] / winfo["mean_diag"]) if winfo["int8"] else 0.0,
                       "vara_kernel_ms": parts["kern"] * 1e3, "prepare_ms": parts["prep"] * 1e3, "certify_ms": parts["cert"] * 1e3,
                       "parity_vara_max_rel_sample": parity["vara_max_rel"] if parity else None,
                       "parity_vara_max_rel_all_markers": all_marker_parity["vara_max_rel_digit_scan_vs_fp64_scan"] if all_marker_parity else None,
                       "parity_gate_passed": parity["gate"]["passed"] if parity else None,
                       "certificate": cert,
                       "operands": "simple" if args.simple_operands else "model algebra on MM^T" + (" (reloaded)" if args.load_operands else "")},
            "rccl_ranks": dist.get_world_size() if world > 1 and backend == "nccl" else 0,   # ranks in the RCCL process group (0: none was made)
            "collective_backend": ("nccl (RCCL)" if backend == "nccl" else backend) if world > 1 else "none (one rank: no collective is issued)",
            "launcher": "self-spawned child torch.distributed.run" if os.environ.get("EAGLE_BENCH_SPAWNED") else ("external launcher" if world > 1 else "single process"),
            "markers_per_rank": [shard_range(Ltot, r, world)[1] - shard_range(Ltot, r, world)[0] for r in range(world)],
            "w_sharing": ("rows 1/%d per rank + one all-gather" % world if world > 1 and sh_share_w else ("replicated on every rank" if world > 1 else "n/a (one rank)")),
            "mmt_build_s": mmt_build_s,
            "mmt_build_breakdown_s": {"fp4 operand image from the marker-major genotypes (k_transpose_pack_fp4)": mmt_image_s,
                                      "partial SYRK (zero + k_syrk_f4w)": syrk_s,
                                      "sum over ranks + mirror / int32 -> fp64 / max + normalise": max(0.0, mmt_build_s - mmt_image_s - syrk_s),
                                      "note": "mmt_build_s is all-in: every pass that exists only for MM^T is inside the timed region"},
            "selected_marker": int(sel[0]), "tsqmax": sel[1],
            "roofline": roof, "roofline_secondary": secondary, "cpu_baseline": cpu, "parity": parity,
            "device": info, "kernel_sha16": sha, "setup_s": {"genotypes": t_gen, "operands": t_ops},
        }
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
