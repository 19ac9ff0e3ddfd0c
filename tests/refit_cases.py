"""The value cases that tests/test_gpu_refit.py runs on the device and tests/test_refit_oracle.py
checks on the oracle alone: each returns the same read-only arrays every time, with the fit
parameters (H, seed, fit threshold) that give the inlier list the case is about."""
import functools

import numpy as np

from match_oracle import MATCH_DT
from ransac_oracle import PLANTED, planted_list

F = np.float32


def _frozen(M):
    M.setflags(write=False)
    return M


def _numbered(M):
    M["query"], M["train"] = np.arange(len(M)), np.arange(len(M))[::-1]
    return M


@functools.lru_cache(maxsize=None)
def exact_list(k, extra=0, seed=0):
    """k records whose train point is an integer affine map of an integer query point (every product
    of the fit is exact, so all k are inliers of the model any four of them give) and `extra` records
    with a train point far from it; shuffled.  The inlier list of a fit that finds the map has
    exactly k records."""
    rng = np.random.default_rng(1000 + 7 * k + extra + seed)
    n = k + extra
    M = np.zeros(n, MATCH_DT)
    x, y = rng.permutation(600)[:n].astype(F), rng.permutation(450)[:n].astype(F)
    M["qx"], M["qy"], M["tx"], M["ty"] = x, y, 2 * x + y + 3, x - y + 7
    M["tx"][k:] += rng.integers(50, 400, extra)
    M["ty"][k:] -= rng.integers(50, 400, extra)
    return _frozen(_numbered(M[rng.permutation(n)]))


@functools.lru_cache(maxsize=None)
def EXTREME():
    """(list, H, seed, fit threshold): every coordinate is +-16383.99, the largest magnitude the rule
    uses.  Four query corners, each with its own train corner (X = -x, Y = y), 75 copies of each:
    |c| reaches 2^23 and the fourth-degree sums 300 * 2^92, so the top limbs of the 128-bit sums and
    their signs are exercised."""
    e = F(16383.99)
    M = np.zeros(300, MATCH_DT)
    sx, sy = np.where(np.arange(300) % 2 == 0, e, -e), np.where(np.arange(300) // 2 % 2 == 0, e, -e)
    M["qx"], M["qy"], M["tx"], M["ty"] = sx, sy, -sx, sy
    return _frozen(_numbered(M)), 256, 1, 3.0


@functools.lru_cache(maxsize=None)
def SKIPPED():
    """(list, H, seed, fit threshold): 200 planted records (140 inliers) with NaN, +-Inf and
    random-byte records mixed in, none of which a fit accepts, and 12 records of the planted map whose
    query point lies beyond 16384: inliers under the loose fit threshold, which the refit skips."""
    rng = np.random.default_rng(21)
    P = planted_list(200, 140, 22)[0].copy()
    P["qx"][::9], P["qy"][2::17], P["ty"][3::11], P["tx"][5::13] = np.nan, -np.inf, np.inf, -np.inf
    R = np.frombuffer(rng.bytes(32 * 40), MATCH_DT).copy()
    far = np.zeros(12, MATCH_DT)
    q = np.stack([rng.uniform(16384.0, 30000.0, 12), rng.uniform(0.0, 480.0, 12)], axis=1)
    p = np.concatenate([q, np.ones((12, 1))], axis=1) @ PLANTED.T
    far["qx"], far["qy"] = q[:, 0], q[:, 1]
    far["tx"], far["ty"] = (p[:, :2] / p[:, 2:]).T
    M = np.concatenate([P, R, far])
    return _frozen(_numbered(M[rng.permutation(len(M))])), 512, 2, 200.0


@functools.lru_cache(maxsize=None)
def TOO_FEW_USED():
    """(list, H, seed, fit threshold): six exact records, three of them beyond 16384: the fit finds
    the map and keeps all six, the refit uses three and has no candidate."""
    M = exact_list(6).copy()
    M["qx"][:3] += 20000
    M["tx"][:3] += 40000
    M["ty"][:3] += 20000
    return _frozen(M), 256, 0, 3.0


@functools.lru_cache(maxsize=None)
def POLLUTED():
    """(list, H, seed, threshold): a fit threshold of 60 px lets gross outliers into the inlier list;
    the least-squares model of that list accepts fewer matches than the RANSAC winner under the same
    threshold, so the round is rejected."""
    return _frozen(planted_list(300, 150, 5, noise=0.5)[0]), 128, 0, 60.0


@functools.lru_cache(maxsize=None)
def NOISY(n, sigma=0.5, seed=0):
    """n planted records, 70 % inliers with `sigma` px of noise."""
    return _frozen(planted_list(n, (7 * n + 9) // 10, 300 + n + seed, noise=sigma)[0])


def planted_points(n=500, seed=1):
    """(query points, their noise-free images under PLANTED) to measure a model against."""
    q = np.random.default_rng(seed).uniform((0.0, 0.0), (640.0, 480.0), (n, 2))
    p = np.concatenate([q, np.ones((n, 1))], axis=1) @ PLANTED.T
    return q, p[:, :2] / p[:, 2:]
