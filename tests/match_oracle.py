"""Literal numpy statement of the descriptor-matching rule of include/gdp.h (gdp_match_descriptors):
the int64 matrix of squared L2 distances between two lists of 176-byte described records, the nearest
train index of every query with ties to the lowest index, the second-smallest distance, the ratio
test in float32, the distance cap, the mutual test and the float32 image coordinates.  Test
infrastructure only; the product path never imports it."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF

# struct gdp_keypoint_oriented / gdp_keypoint_described / gdp_match_record, restated here so that the
# oracle does not depend on the package under test
_ORIENTED = [("octave", np.uint16, 0), ("scale", np.uint8, 2), ("kind", np.int8, 3), ("row", np.int32, 4), ("col", np.int32, 8),
             ("value", F, 12), ("dscale", F, 16), ("drow", F, 20), ("dcol", F, 24), ("interp", F, 28), ("angle", F, 32),
             ("peak", F, 36), ("bin", np.uint32, 40), ("peaks", np.uint32, 44)]
DESCRIBED_DT = np.dtype({"names": [n for n, _, _ in _ORIENTED] + ["desc"],
                         "formats": [t for _, t, _ in _ORIENTED] + [(np.uint8, (128,))],
                         "offsets": [o for _, _, o in _ORIENTED] + [48], "itemsize": 176})
MATCH_DT = np.dtype({"names": ["query", "train", "distance", "second", "qx", "qy", "tx", "ty"],
                     "formats": [np.uint32] * 4 + [F] * 4, "offsets": [0, 4, 8, 12, 16, 20, 24, 28], "itemsize": 32})


def distances(Q, T):
    """dist[i, j] = sum_k (Q[i].desc[k] - T[j].desc[k])^2 as int64, in blocks of query rows (a
    difference squared is at most 65,025 and a sum at most 8,323,200: int32 holds both exactly)."""
    q = np.asarray(Q["desc"], np.int32).reshape(len(Q), 128)
    t = np.asarray(T["desc"], np.int32).reshape(len(T), 128)
    out = np.zeros((len(q), len(t)), np.int64)
    for i in range(0, len(q), 16):
        d = q[i:i + 16, None, :] - t[None, :, :]
        out[i:i + 16] = (d * d).sum(axis=2)
    return out


def coordinates(R):
    """(x, y) of every record: sc = (float)(1u << (octave & 31)), x = ((float)col + dcol) * sc,
    y = ((float)row + drow) * sc, each operation rounded to float32."""
    sc = (np.uint32(1) << (R["octave"].astype(np.uint32) & np.uint32(31))).astype(F)
    x = (R["col"].astype(F) + R["dcol"].astype(F)) * sc
    y = (R["row"].astype(F) + R["drow"].astype(F)) * sc
    return x.astype(F), y.astype(F)


def np_match(Q, T, ratio=0.0, max_distance=NONE, mutual=False, D=None):
    """The rule applied literally; a MATCH_DT array sorted by `query`.  `D`: distances(Q, T) when
    the caller already has it (several filters over the same two lists)."""
    Q = np.asarray(Q, DESCRIBED_DT).reshape(-1)
    T = np.asarray(T, DESCRIBED_DT).reshape(-1)
    nq, nt = len(Q), len(T)
    out = np.zeros(nq, MATCH_DT)
    if nq == 0 or nt == 0:
        return out[:0]
    D = distances(Q, T) if D is None else D
    assert D.shape == (nq, nt) and D.dtype == np.int64
    with np.errstate(invalid="ignore"):
        qx, qy = coordinates(Q)
        tx, ty = coordinates(T)
    r2 = F(ratio) * F(ratio)
    nearest_query = D.argmin(axis=0)  # of every train: the first minimum is the lowest query index
    n = 0
    for i in range(nq):
        row = D[i]
        j = int(row.argmin())  # the first minimum: ties go to the lowest index
        distance = int(row[j])
        second = int(np.delete(row, j).min()) if nt > 1 else NONE
        if ratio != 0 and not (F(distance) < r2 * F(second)):
            continue
        if not distance <= max_distance:
            continue
        if mutual and int(nearest_query[j]) != i:
            continue
        out[n] = (i, j, distance, second, qx[i], qy[i], tx[j], ty[j])
        n += 1
    return out[:n]
