"""Literal numpy statement of the guided-matching rule of include/gdp.h (gdp_match_guided): the float32
coordinates of both lists, the projection of every query under nine floats with separately rounded
operations and two correctly rounded divisions, the square window, the candidate matrix of four
comparisons per pair over ALL pairs (brute force: no grid, so it shares no structure with the kernel),
the nearest and second-nearest candidate, the ratio test, the cap and the `unique` step.  Test
infrastructure only; the product path never imports it."""
import numpy as np

from match_oracle import DESCRIBED_DT, MATCH_DT, NONE, coordinates, distances

F = np.float32


def windows(Q, h, radius):
    """(x0, x1, y0, y1, has) per query: steps 2 and 3; `has` is False where !(w > 0)."""
    h = np.asarray(h, F).reshape(9)
    r = F(radius)
    with np.errstate(all="ignore"):
        qx, qy = coordinates(Q)
        u = (h[0] * qx + h[1] * qy).astype(F) + h[2]
        v = (h[3] * qx + h[4] * qy).astype(F) + h[5]
        w = (h[6] * qx + h[7] * qy).astype(F) + h[8]
        has = w > 0
        sx, sy = (u / w).astype(F), (v / w).astype(F)
        return (sx - r).astype(F), (sx + r).astype(F), (sy - r).astype(F), (sy + r).astype(F), has


def candidates(Q, T, h, radius):
    """C[i, j]: train j is a candidate of query i (step 4), a bool matrix over all pairs."""
    x0, x1, y0, y1, has = windows(Q, h, radius)
    with np.errstate(invalid="ignore"):
        tx, ty = coordinates(T)
        return (has[:, None] & (x0[:, None] <= tx[None, :]) & (tx[None, :] <= x1[:, None]) & (y0[:, None] <= ty[None, :]) &
                (ty[None, :] <= y1[:, None]))


def np_guided(Q, T, h, radius, ratio=0.0, max_distance=NONE, unique=True, D=None, stats=None):
    """The rule applied literally; a MATCH_DT array sorted by `query`.  `D`: distances(Q, T) when the
    caller already has it.  `stats`, a dict, receives what the tests' non-vacuity conditions need:
    'multi' (queries with two or more candidates), 'ratio_dropped', 'unique_dropped'."""
    Q = np.asarray(Q, DESCRIBED_DT).reshape(-1)
    T = np.asarray(T, DESCRIBED_DT).reshape(-1)
    nq, nt = len(Q), len(T)
    out = np.zeros(nq, MATCH_DT)
    stats = {} if stats is None else stats
    stats.update(multi=0, ratio_dropped=0, unique_dropped=0)
    if nq == 0 or nt == 0:
        return out[:0]
    D = distances(Q, T) if D is None else D
    assert D.shape == (nq, nt) and D.dtype == np.int64
    C = candidates(Q, T, h, radius)
    with np.errstate(invalid="ignore"):
        qx, qy = coordinates(Q)
        tx, ty = coordinates(T)
    r2 = F(ratio) * F(ratio)
    big = np.int64(1) << 40
    kept = []
    for i in range(nq):
        n = int(C[i].sum())
        if n == 0:
            continue
        stats["multi"] += n >= 2
        row = np.where(C[i], D[i], big)
        j = int(row.argmin())  # the first minimum: ties go to the lowest index
        distance = int(row[j])
        second = int(np.delete(row, j).min()) if n > 1 else NONE
        if ratio != 0 and not (F(distance) < r2 * F(second)):
            stats["ratio_dropped"] += 1
            continue
        if not distance <= max_distance:
            continue
        kept.append((i, j, distance, second))
    if unique:
        best = {}
        for i, j, distance, _ in kept:
            if j not in best or (distance, i) < best[j]:
                best[j] = (distance, i)
        stats["unique_dropped"] = sum(best[j] != (distance, i) for i, j, distance, _ in kept)
        kept = [k for k in kept if best[k[1]] == (k[2], k[0])]
    for n, (i, j, distance, second) in enumerate(kept):
        out[n] = (i, j, distance, second, qx[i], qy[i], tx[j], ty[j])
    return out[:len(kept)]
