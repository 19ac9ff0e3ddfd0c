"""The matching oracle (tests/match_oracle.py) against a pure-Python double loop on small lists that
contain ties, and its extremes; no GPU, no library."""
import numpy as np

from match_oracle import DESCRIBED_DT, MATCH_DT, NONE, F, coordinates, distances, np_match


def tied_lists():
    """7 queries x 5 trains over three distinct descriptors: ties on both axes."""
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (3, 128), dtype=np.uint8)
    Q, T = np.zeros(7, DESCRIBED_DT), np.zeros(5, DESCRIBED_DT)
    Q["desc"] = base[[0, 1, 0, 2, 1, 0, 2]]
    T["desc"] = base[[1, 0, 1, 0, 0]]
    T["desc"][4, 7] ^= 1  # train 4 is one step away from train 1 and train 3
    for R, seed in ((Q, 1), (T, 2)):
        r = np.random.default_rng(seed)
        R["octave"] = r.integers(0, 4, len(R))
        R["row"], R["col"] = r.integers(0, 40, len(R)), r.integers(0, 56, len(R))
        R["drow"], R["dcol"] = r.uniform(-0.5, 0.5, len(R)).astype(F), r.uniform(-0.5, 0.5, len(R)).astype(F)
    return Q, T


def loop_match(Q, T, ratio, max_distance, mutual):
    """The rule as two plain loops over Python ints."""
    dist = [[sum((int(a) - int(b)) ** 2 for a, b in zip(q["desc"], t["desc"])) for t in T] for q in Q]
    out = []
    for i in range(len(Q)):
        if not len(T):
            continue
        j = min(range(len(T)), key=lambda k: (dist[i][k], k))
        second = min((dist[i][k] for k in range(len(T)) if k != j), default=NONE)
        if ratio != 0 and not (F(dist[i][j]) < (F(ratio) * F(ratio)) * F(second)):
            continue
        if dist[i][j] > max_distance:
            continue
        if mutual and min(range(len(Q)), key=lambda k: (dist[k][j], k)) != i:
            continue
        out.append((i, j, dist[i][j], second))
    return out


def test_oracle_equals_the_double_loop_on_lists_with_ties():
    Q, T = tied_lists()
    D = distances(Q, T)
    assert D.dtype == np.int64 and D.shape == (7, 5)
    assert (D == 0).sum() >= 8 and D[0, 4] == 1  # ties and a near-tie are really there
    seen = set()
    for ratio in (0.0, 0.8, 1.0):
        for cap in (NONE, 0, 1):
            for mutual in (False, True):
                got = np_match(Q, T, ratio, cap, mutual)
                assert got.dtype == MATCH_DT
                want = loop_match(Q, T, ratio, cap, mutual)
                assert [tuple(int(r[f]) for f in ("query", "train", "distance", "second")) for r in got] == want, (ratio, cap, mutual)
                seen.add(len(want))
    assert len(seen) > 2
    got = np_match(Q, T)  # no test at all: one record per query, lowest index on a tie, second == distance
    assert list(got["query"]) == list(range(7))
    assert list(got["train"][[0, 2, 5]]) == [1, 1, 1] and list(got["train"][[1, 4]]) == [0, 0]
    assert (got["second"][[0, 1, 2, 4, 5]] == got["distance"][[0, 1, 2, 4, 5]]).all() and (got["distance"][[0, 1, 2, 4, 5]] == 0).all()
    mutual = np_match(Q, T, mutual=True)  # duplicate queries keep only the lowest
    assert [(int(r["query"]), int(r["train"])) for r in mutual if r["distance"] == 0] == [(0, 1), (1, 0)]
    qx, qy = coordinates(Q)
    tx, ty = coordinates(T)
    for r in got:
        i, j = int(r["query"]), int(r["train"])
        sq, st = F(1 << int(Q["octave"][i])), F(1 << int(T["octave"][j]))
        assert r["qx"] == (F(Q["col"][i]) + Q["dcol"][i]) * sq == qx[i] and r["qy"] == (F(Q["row"][i]) + Q["drow"][i]) * sq == qy[i]
        assert r["tx"] == (F(T["col"][j]) + T["dcol"][j]) * st == tx[j] and r["ty"] == (F(T["row"][j]) + T["drow"][j]) * st == ty[j]


def test_extremes():
    Q, T = np.zeros(1, DESCRIBED_DT), np.zeros(1, DESCRIBED_DT)
    T["desc"] = 255
    got = np_match(Q, T)
    assert len(got) == 1 and got["distance"][0] == 8323200 == 128 * 255 * 255 and got["second"][0] == NONE  # nt = 1
    assert len(np_match(Q, T, ratio=0.8)) == 1  # (float)0xffffffff is 2^32: 8323200 < 0.64 * 2^32
    assert len(np_match(Q, T, max_distance=8323200)) == 1 and len(np_match(Q, T, max_distance=8323199)) == 0
    assert len(np_match(Q, T[:0])) == 0 and len(np_match(Q[:0], T)) == 0  # nt = 0: nothing; nq = 0: nothing
    Q["octave"], Q["row"], Q["col"], Q["drow"], Q["dcol"] = 33, 3, 5, 0.25, -0.5  # the octave is taken & 31
    got = np_match(Q, T)
    assert got["qx"][0] == 9.0 and got["qy"][0] == 6.5 and got["tx"][0] == 0.0
