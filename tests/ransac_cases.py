"""The value cases that tests/test_gpu_ransac.py runs on the device and tests/test_ransac_oracle.py
checks on the oracle alone: each returns the same read-only arrays every time."""
import functools

import numpy as np

from match_oracle import MATCH_DT
from ransac_oracle import planted_list


def _frozen(M):
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def TIE():
    """(list, H, seed): 150 planted inliers of 200 at a noise far below the threshold, so that every
    hypothesis sampled from inliers alone accepts exactly the 150: a tie between many."""
    return _frozen(planted_list(200, 150, 11)[0]), 128, 0


@functools.lru_cache(maxsize=None)
def NO_VALID():
    """(list, H, seed): four records and eight hypotheses none of which draws four distinct indices
    (a draw is a permutation of four with probability 4!/4^4 = 9.4 %; this seed has none in eight)."""
    return _frozen(planted_list(4, 4, 12)[0]), 8, 3


@functools.lru_cache(maxsize=None)
def collinear_list(n):
    """Even records have their query point on the line y = 2x + 1, odd records anywhere; all integer
    coordinates, the train point an integer affine map of the query point, so every product of the
    fit is exact: a sample of four points on the line gives lambda = 0 and an all-zero matrix, one
    with three of them a singular matrix."""
    rng = np.random.default_rng(13)
    M = np.zeros(n, MATCH_DT)
    x = rng.permutation(4 * n)[:n].astype(np.float32)
    y = np.where(np.arange(n) % 2 == 0, 2 * x + 1, rng.integers(0, 500, n)).astype(np.float32)
    M["qx"], M["qy"], M["tx"], M["ty"] = x, y, 2 * x + y + 3, x - y + 7
    M["query"], M["train"] = np.arange(n), np.arange(n)
    return _frozen(M)
