"""The refit rule of include/gdp.h (gdp_refit_homography) applied literally: Python integers for
steps 1 to 4 (quantisation, origin, the 24 moment sums, the scale exponents), scalar numpy float64,
one operation per rounded operation of the rule, for steps 5 and 6, and ransac_oracle's float32
scoring for step 7.  No sum(), dot or @ over the rule's float arithmetic: their order is not fixed."""
import numpy as np

from match_oracle import MATCH_DT
from ransac_oracle import F, NONE, inlier_mask

D = np.float64

# struct gdp_refit_record, restated here so that the package's dtype is compared with something
REFIT_DT = np.dtype({"names": ["rounds", "accepted", "used", "skipped", "count_before", "count_after", "status", "kq", "kt",
                               "origin", "h", "reserved"],
                     "formats": [np.uint32] * 9 + [(np.int32, 4), (F, 9), (np.uint32, 2)],
                     "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 52, 88], "itemsize": 96})

ACCEPTED, TOO_FEW, PIVOT, NON_FINITE, FEWER, NO_MODEL = 1, 2, 3, 4, 5, 6
LIMIT = F(16384.0)
DEG_Q, DEG_T = (0, 1, 1, 2, 2, 2), (0, 1, 1, 2)


def quantise(L):
    """Step 1: (q as a list of four-tuples of Python integers for the used records, skipped)."""
    f = np.stack([np.ascontiguousarray(L[k]) for k in ("qx", "qy", "tx", "ty")], axis=1) if len(L) else np.zeros((0, 4), F)
    assert f.dtype == F
    with np.errstate(all="ignore"):
        used = np.all(np.abs(f) < LIMIT, axis=1)  # False for a NaN and an infinity
        p = f[used] * F(256.0)
        assert p.dtype == F
        q = np.rint(p).astype(np.int64)
    return [tuple(int(v) for v in row) for row in q], int(len(L) - np.count_nonzero(used))


def moments(q, o):
    """Step 3: mu[a][b] as Python integers."""
    mu = [[0] * 4 for _ in range(6)]
    for rec in q:
        cx, cy, cX, cY = (rec[k] - o[k] for k in range(4))
        mono = (1, cx, cy, cx * cx, cx * cy, cy * cy)
        tmono = (1, cX, cY, cX * cX + cY * cY)
        for a in range(6):
            for b in range(4):
                mu[a][b] += mono[a] * tmono[b]
    return mu


def scale(total, used):
    """Step 4: the smallest k >= 0 with total < used * 4^k."""
    k = 0
    while not total < used * 4 ** k:
        k += 1
    return k


def to_double(v, shift):
    """Step 5's conversion of a 128-bit sum."""
    m = abs(v)
    assert m < 1 << 127
    d = D(float(m >> 64)) * D(18446744073709551616.0) + D(float(m & ((1 << 64) - 1)))  # int -> float is to nearest even
    return np.ldexp(-d if v < 0 else d, -shift)


def normal_equations(mu, kq, kt):
    """(the lower triangle of N with every other entry +0, rhs) of step 5."""
    S = [[to_double(mu[a][b], kq * DEG_Q[a] + kt * DEG_T[b]) for b in range(4)] for a in range(6)]
    N = [[D(0.0)] * 8 for _ in range(8)]
    rhs = [D(0.0)] * 8
    P = [[S[3][0], S[4][0], S[1][0]], [S[4][0], S[5][0], S[2][0]], [S[1][0], S[2][0], S[0][0]]]
    for i in range(3):
        for j in range(i + 1):
            N[i][j] = N[3 + i][3 + j] = P[i][j]
    for b, c in ((1, 0), (2, 3)):
        N[6][c], N[6][c + 1], N[6][c + 2] = -S[3][b], -S[4][b], -S[1][b]
        N[7][c], N[7][c + 1], N[7][c + 2] = -S[4][b], -S[5][b], -S[2][b]
        rhs[c], rhs[c + 1], rhs[c + 2] = S[1][b], S[2][b], S[0][b]
    N[6][6], N[7][6], N[7][7] = S[3][3], S[4][3], S[5][3]
    rhs[6], rhs[7] = -S[1][3], -S[2][3]
    return N, rhs


def solve(N, rhs):
    """Step 5's LDL^T without pivoting: g[0..8), or None at a pivot that is not > 0."""
    Lm = [[D(0.0)] * 8 for _ in range(8)]
    Dg = [D(0.0)] * 8
    for j in range(8):
        v = [Lm[j][k] * Dg[k] for k in range(j)]
        d = N[j][j]
        for k in range(j):
            d = d - Lm[j][k] * v[k]
        Dg[j] = d
        if not d > 0.0:
            return None
        for i in range(j + 1, 8):
            e = N[i][j]
            for k in range(j):
                e = e - Lm[i][k] * v[k]
            Lm[i][j] = e / d
    z = [D(0.0)] * 8
    for i in range(8):
        e = rhs[i]
        for k in range(i):
            e = e - Lm[i][k] * z[k]
        z[i] = e
    g = [D(0.0)] * 8
    for i in range(7, -1, -1):
        e = z[i] / Dg[i]
        for k in range(i + 1, 8):
            e = e - Lm[k][i] * g[k]
        g[i] = e
    return g


def denormalise(g, o, kq, kt):
    """Step 6: the nine float32 of the candidate, or None when it is not finite."""
    a, bx, by = np.ldexp(D(256.0), -kq), np.ldexp(-D(float(o[0])), -kq), np.ldexp(-D(float(o[1])), -kq)
    sc, tX, tY = np.ldexp(D(1.0), kt - 8), D(float(o[2])) / D(256.0), D(float(o[3])) / D(256.0)
    Hh = [[g[0], g[1], g[2]], [g[3], g[4], g[5]], [g[6], g[7], D(1.0)]]
    K = [[Hh[r][0] * a, Hh[r][1] * a, (Hh[r][0] * bx + Hh[r][1] * by) + Hh[r][2]] for r in range(3)]
    G = [[sc * K[0][c] + tX * K[2][c] for c in range(3)], [sc * K[1][c] + tY * K[2][c] for c in range(3)], [K[2][c] for c in range(3)]]
    s, nan = D(0.0), False
    for r in range(3):
        for c in range(3):
            assert G[r][c].dtype == D
            m = np.abs(G[r][c])
            nan = nan or bool(np.isnan(m))
            s = m if m > s else s
    if nan or not (s > 0.0 and np.isfinite(s)):
        return None
    _, e = np.frexp(s)
    return np.array([np.ldexp(G[r][c], -int(e)) for r in range(3) for c in range(3)], D).astype(F)


def candidate(L):
    """Steps 1-6 on the inlier list L: a dict with status (0: a candidate exists), used, skipped, kq,
    kt, origin and h (nine float32, all 0 without a candidate)."""
    q, skipped = quantise(L)
    out = {"status": 0, "used": len(q), "skipped": skipped, "kq": 0, "kt": 0, "origin": (0, 0, 0, 0), "h": np.zeros(9, F)}
    if len(q) < 4:
        out["status"] = TOO_FEW
        return out
    used = len(q)
    o = tuple(sum(rec[k] for rec in q) // used for k in range(4))  # // rounds toward -infinity
    mu = moments(q, o)
    for row in mu:
        for v in row:
            assert abs(v) < 1 << 125
    kq, kt = scale(mu[3][0] + mu[5][0], used), scale(mu[0][3], used)
    out.update(kq=kq, kt=kt, origin=o)
    with np.errstate(all="ignore"):
        g = solve(*normal_equations(mu, kq, kt))
        if g is None:
            out["status"] = PIVOT
            return out
        h = denormalise(g, o, kq, kt)
    if h is None:
        out["status"] = NON_FINITE
    else:
        out["h"] = h
    return out


def count(h, M, threshold):
    """The fit rule's step 5 under the nine float32 h: (the count, the mask)."""
    tt = F(threshold) * F(threshold)
    mask = inlier_mask([F(v) for v in h], M["qx"], M["qy"], M["tx"], M["ty"], tt)
    return int(np.count_nonzero(mask)), mask


def np_refit(M, model, inliers, rounds=1, threshold=3.0):
    """(the model record, the inliers sorted by `query`, the refit record) after `rounds` rounds on
    the list M, the model record `model` and the inlier list `inliers` (in any order)."""
    M = np.ascontiguousarray(M, MATCH_DT)
    model, L = np.array(model).copy(), np.ascontiguousarray(inliers, MATCH_DT)
    rec = np.zeros((), REFIT_DT)
    rec["rounds"] = rounds
    if int(model["hypothesis"]) == NONE:
        rec["status"] = NO_MODEL
        return model, L, rec
    for r in range(rounds):
        cand = candidate(L)
        c_cur, _ = count(model["h"], M, threshold)
        c_new, mask = count(cand["h"], M, threshold)
        assert cand["status"] == 0 or c_new == 0  # h[] = 0 gives w = 0
        accept = cand["status"] == 0 and c_new >= c_cur and c_new >= 4
        if r == 0:
            rec["count_before"] = c_cur
        rec["used"], rec["skipped"], rec["kq"], rec["kt"] = cand["used"], cand["skipped"], cand["kq"], cand["kt"]
        rec["origin"], rec["h"] = cand["origin"], cand["h"]
        rec["status"] = cand["status"] or (ACCEPTED if accept else FEWER)
        if not accept:
            break
        rec["accepted"] += 1
        model["h"], model["inliers"], model["matches"] = cand["h"], c_new, len(M)
        L = M[mask]
    rec["count_after"] = model["inliers"]
    L = L[np.argsort(L["query"], kind="stable")]
    return model, L, rec


def transfer_rms(h, q, t):
    """RMS distance in pixels between h applied to the points q[n][2] and t[n][2], in float64."""
    h = np.asarray(h, D).reshape(3, 3)
    p = np.concatenate([np.asarray(q, D), np.ones((len(q), 1))], axis=1) @ h.T
    return float(np.sqrt(np.mean(np.sum((p[:, :2] / p[:, 2:] - np.asarray(t, D)) ** 2, axis=1))))
