"""Helpers of the line-score tests (tests/test_scores_host.py, test_scores_abi.py, test_gpu_scores.py): truths written from the
definition of include/eagle_hip.h section 1b''''i in numpy and Python integers.  No device, and no code of the feature."""
import functools

import numpy as np

W30 = 1 << 30
EDGES = (0, 1, -1, 127, 128, -128, -129, 32639, 32640, -32896, -32897, 8355711, 8355712, -8421504, -8421505, W30 - 1, W30, -W30)
EPS = float(np.finfo(np.float64).eps)


def np_scores(G8, w):
    """out[r, t] = sum_c w[t, c] G8[r, c] in int64; G8 (R, C) in {-1, 0, +1}, w (T, C) integers of at most 2^30 in magnitude."""
    return np.asarray(G8).astype(np.int64) @ np.atleast_2d(np.asarray(w)).astype(np.int64).T


def py_scores(G8, w):
    """The same as a Python-int double loop (small cases only)."""
    G8, w = np.asarray(G8), np.atleast_2d(np.asarray(w))
    return np.array([[sum(int(w[t, c]) * int(G8[r, c]) for c in range(G8.shape[1])) for t in range(w.shape[0])] for r in range(G8.shape[0])],
                    dtype=np.int64)


def edge_weights(T, C, seed):
    """(T, C) int64 weights in +-2^30: every column cycles through EDGES in its first positions (shifted by its index, so that the columns
    differ) and is random after; column 1 (when there is one) has |w| <= 127 (one digit plane), column 2 multiples of 256 (plane 0
    empty), column 3 is zero."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-W30, W30 + 1, (T, C))
    k = min(C, 3 * len(EDGES))
    for t in range(T):
        w[t, :k] = np.resize(np.roll(np.array(EDGES, dtype=np.int64), t), k)
    if T > 1:
        w[1] = rng.integers(-127, 128, C)
    if T > 2:
        w[2] = rng.integers(-(1 << 22), (1 << 22) + 1, C) * 256
    if T > 3:
        w[3] = 0
    return w


@functools.lru_cache(maxsize=None)
def edge_panel():
    """M8 int8 (1003, 5000): the M file has 1,003 lines of 5,000, the Mt file 5,000 lines of 1,003 -- line counts that cross 256, 512
    and 768, lengths that are no multiple of 128.  Read-only."""
    from eagleeverything_amd import synth
    M8 = np.ascontiguousarray(synth.genotypes_marker_major(1003, 5000, seed=4321).T)
    M8.setflags(write=False)
    return M8


def k_splits(C):
    """(stages, splits) of a line of C characters under the launch rule of the Gram engine: 128-byte K stages, splits of at least 16
    stages, as many as about 10 waves of 256 workgroups want (far more than the few row tiles of the test panels leave)."""
    stages = -(-C // 128)
    return stages, max(stages // 16, 1)


def dot_bound(a, b):
    """The standard bound of an fp64 dot product of len(a) terms, |fl(a.b) - a.b| <= gamma_n sum |a_i b_i| (Higham, Accuracy and
    Stability, section 3.1), with gamma_n = n eps / (1 - n eps)."""
    n = a.shape[-1]
    return n * EPS / (1.0 - n * EPS) * float(np.max(np.abs(a) @ np.abs(b)))
