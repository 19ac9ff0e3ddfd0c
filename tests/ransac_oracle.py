"""The RANSAC homography rule of include/gdp.h (gdp_fit_homography) applied literally in numpy, one
array operation per rounded operation of the rule: uint32 / uint64 for the sampler, float64 for the
four-point fit, float32 for the scoring.  No einsum, no @, no sum over the rule's float arithmetic:
their order is not fixed.  All H hypotheses are carried through every step as arrays of length H."""
import numpy as np

from match_oracle import MATCH_DT

F = np.float32
NONE = 0xFFFFFFFF

# struct gdp_homography, restated here so that the package's dtype is compared with something
HOMOGRAPHY_DT = np.dtype({"names": ["h", "hypothesis", "inliers", "matches", "sample"],
                          "formats": [(F, 9), np.uint32, np.uint32, np.uint32, (np.uint32, 4)],
                          "offsets": [0, 36, 40, 44, 48], "itemsize": 64})

_M32 = np.uint64(0xFFFFFFFF)


def mix(x):
    """Step 1's mixer on an array of uint32 values (held in uint64, masked after every product)."""
    x = np.asarray(x, np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def sample(n, H, seed):
    """(idx[H][4] as uint32, valid[H]): step 1."""
    h = np.arange(H, dtype=np.uint64)[:, None]
    k = np.arange(4, dtype=np.uint64)[None, :]
    arg = (np.uint64(seed) + ((np.uint64(0x9E3779B9) * ((np.uint64(4) * h + k + np.uint64(1)) & _M32)) & _M32)) & _M32
    idx = (mix(arg) * np.uint64(n)) >> np.uint64(32)
    valid = np.full(H, n >= 4)
    for a in range(4):
        for b in range(a + 1, 4):
            valid &= idx[:, a] != idx[:, b]
    return idx.astype(np.uint32), valid


def adj(M):
    """The nine expressions of step 2 in the header's order; M[r][c] are float64 arrays."""
    return [[M[1][1] * M[2][2] - M[1][2] * M[2][1], M[0][2] * M[2][1] - M[0][1] * M[2][2], M[0][1] * M[1][2] - M[0][2] * M[1][1]],
            [M[1][2] * M[2][0] - M[1][0] * M[2][2], M[0][0] * M[2][2] - M[0][2] * M[2][0], M[0][2] * M[1][0] - M[0][0] * M[1][2]],
            [M[1][0] * M[2][1] - M[1][1] * M[2][0], M[0][1] * M[2][0] - M[0][0] * M[2][1], M[0][0] * M[1][1] - M[0][1] * M[1][0]]]


def basis(x, y):
    """Step 2: x[k], y[k] are the float64 arrays of sample point k."""
    one = np.ones_like(x[0])
    M = [[x[0], x[1], x[2]], [y[0], y[1], y[2]], [one, one, one]]
    J = adj(M)
    lam = [(J[r][0] * x[3] + J[r][1] * y[3]) + J[r][2] for r in range(3)]
    return [[M[r][c] * lam[c] for c in range(3)] for r in range(3)]


def fit(M, H, seed):
    """Steps 1-4: the H hypothesis records with inliers = 0."""
    n = len(M)
    idx, valid = sample(n, H, seed)
    out = np.zeros(H, HOMOGRAPHY_DT)
    out["hypothesis"], out["matches"], out["sample"] = np.arange(H), n, idx
    if n < 4:
        return out
    with np.errstate(all="ignore"):
        pt = {f: [M[f][idx[:, k]].astype(np.float64) for k in range(4)] for f in ("qx", "qy", "tx", "ty")}
        assert all(a.dtype == np.float64 for v in pt.values() for a in v)
        A, B = basis(pt["qx"], pt["qy"]), basis(pt["tx"], pt["ty"])
        J = adj(A)
        G = [[(B[r][0] * J[0][c] + B[r][1] * J[1][c]) + B[r][2] * J[2][c] for c in range(3)] for r in range(3)]
        s, nan = np.zeros(H), np.zeros(H, bool)
        for r in range(3):
            for c in range(3):
                a = np.abs(G[r][c])
                nan |= np.isnan(a)
                s = np.where(a > s, a, s)  # a NaN never becomes s
        valid = valid & ~nan & (s > 0) & np.isfinite(s)
        _, e = np.frexp(np.where(valid, s, 1.0))
        G = [[np.ldexp(G[r][c], -e) for c in range(3)] for r in range(3)]
        w0 = (G[2][0] * pt["qx"][0] + G[2][1] * pt["qy"][0]) + G[2][2]
        flip = w0 < 0
        for r in range(3):
            for c in range(3):
                g = np.where(flip, -G[r][c], G[r][c])
                assert g.dtype == np.float64
                out["h"][:, 3 * r + c] = np.where(valid, g, 0.0).astype(F)  # round to nearest even, denormals kept
    return out


def inlier_mask(h, x, y, X, Y, tt):
    """Step 5 in float32: h[k] broadcast against the coordinates."""
    with np.errstate(all="ignore"):
        u = (h[0] * x + h[1] * y) + h[2]
        v = (h[3] * x + h[4] * y) + h[5]
        w = (h[6] * x + h[7] * y) + h[8]
        dx = X * w - u
        dy = Y * w - v
        e = dx * dx + dy * dy
        bound = tt * (w * w)
        for a in (u, v, w, dx, dy, e, bound):
            assert a.dtype == F
        return (w > 0) & (e <= bound)


def score(hyp, M, threshold, block=256):
    """Step 5: the count of every hypothesis (an integer sum of booleans)."""
    tt = F(threshold) * F(threshold)
    assert tt.dtype == F
    x, y, X, Y = (np.ascontiguousarray(M[f])[None, :] for f in ("qx", "qy", "tx", "ty"))
    counts = np.zeros(len(hyp), np.int64)
    for h0 in range(0, len(hyp), block):
        h = [np.ascontiguousarray(hyp["h"][h0:h0 + block, k])[:, None] for k in range(9)]
        counts[h0:h0 + block] = np.count_nonzero(inlier_mask(h, x, y, X, Y, tt), axis=1)
    return counts


def none_record(n):
    r = np.zeros(1, HOMOGRAPHY_DT)
    r["hypothesis"], r["matches"], r["sample"] = NONE, n, NONE
    return r[0]


def np_ransac(M, H, seed=0, threshold=3.0, min_inliers=4):
    """(the H hypothesis records, the model record, the inliers sorted by `query`)."""
    M = np.ascontiguousarray(M, MATCH_DT)
    hyp = fit(M, H, seed)
    counts = score(hyp, M, threshold)
    valid = np.any(hyp["h"] != 0, axis=1)
    assert not counts[~valid].any()  # h[] = 0 gives w = 0
    hyp["inliers"] = counts
    model, inliers = none_record(len(M)), M[:0]
    if valid.any():
        win = int(np.argmax(np.where(valid, counts, -1)))  # the first of the largest: ties to the lowest h
        if counts[win] >= max(int(min_inliers), 4):
            model = hyp[win].copy()
            tt = F(threshold) * F(threshold)
            mask = inlier_mask([F(v) for v in model["h"]], M["qx"], M["qy"], M["tx"], M["ty"], tt)
            assert np.count_nonzero(mask) == counts[win]
            inliers = M[mask]
            inliers = inliers[np.argsort(inliers["query"], kind="stable")]
    return hyp, model, inliers


def matrix(model):
    """The 3 x 3 float32 array of a model record, or None when it holds no model."""
    return None if int(model["hypothesis"]) == NONE else np.array(model["h"], F).reshape(3, 3)


# A fixed projective transform of a 640 x 480 image: rotation, anisotropic scale, shift, perspective
PLANTED = np.array([[0.9, -0.2, 30.0], [0.25, 1.1, -12.0], [1e-4, -5e-5, 1.0]])


def planted_list(n, inliers, seed, noise=0.1):
    """(n records, the planted mask): `inliers` of them are a query point mapped by PLANTED plus
    Gaussian noise of `noise` pixels, the rest uniform pairs; shuffled.  `query` numbers the records,
    so the sorted download is the list's own order."""
    rng = np.random.default_rng(seed)
    q = rng.uniform((0.0, 0.0), (640.0, 480.0), (n, 2))
    p = np.concatenate([q, np.ones((n, 1))], axis=1) @ PLANTED.T
    t = p[:, :2] / p[:, 2:] + rng.normal(0.0, noise, (n, 2))
    planted = np.arange(n) < inliers
    t[~planted] = rng.uniform((-100.0, -100.0), (800.0, 700.0), (n - inliers, 2))
    order = rng.permutation(n)
    M = np.zeros(n, MATCH_DT)
    M["qx"], M["qy"], M["tx"], M["ty"] = q[order, 0], q[order, 1], t[order, 0], t[order, 1]
    M["query"], M["train"] = np.arange(n), rng.permutation(n)
    M["distance"] = rng.integers(0, 40000, n)
    M["second"] = M["distance"] + rng.integers(0, 40000, n)
    return M, planted[order]
