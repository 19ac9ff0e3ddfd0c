"""The warp rule of include/gdp.h (gdp_warp_image) applied literally in numpy, all pixels at once, one
array operation per rounded operation of the rule: float64 for the adjugate of step 1, np.float32 for
steps 2 and 3.  np.rint, np.floor and float32 `/` are the rule's operations (ties to even, floorf, the
IEEE correctly rounded division)."""
import numpy as np

from ransac_oracle import NONE, adj

F = np.float32
TRAIN_TO_QUERY, QUERY_TO_TRAIN = 0, 1

# struct gdp_warp_record, restated here so that the package's dtype is compared with something
WARP_DT = np.dtype({"names": ["m", "model", "covered", "pixels", "sad", "direction", "reserved"],
                    "formats": [(F, 9), np.uint32, np.uint32, np.uint32, np.uint64, np.uint32, np.uint32],
                    "offsets": [0, 36, 40, 44, 48, 56, 60], "itemsize": 64})

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def matrix(h, direction, none=False):
    """Step 1: (m[9] as float32, model).  `h` is nine float32; none=True: the model record says "none"."""
    h = np.asarray(h, F).reshape(9)
    zero = np.zeros(9, F)
    if none:
        return zero, 0
    if direction == TRAIN_TO_QUERY:
        return h.copy(), 1
    with np.errstate(all="ignore"):
        M = [[np.float64(h[3 * r + c]) for c in range(3)] for r in range(3)]
        G = adj(M)
        det = (M[0][0] * G[0][0] + M[0][1] * G[1][0]) + M[0][2] * G[2][0]
        s, nan = np.float64(0.0), False
        for r in range(3):
            for c in range(3):
                a = np.abs(G[r][c])
                nan = nan or bool(np.isnan(a))
                s = a if a > s else s  # a NaN never becomes s
        if nan or not s > 0 or not np.isfinite(s) or np.isnan(det) or det == 0:
            return zero, 0
        _, e = np.frexp(s)
        m = np.zeros(9, F)
        for r in range(3):
            for c in range(3):
                g = np.ldexp(G[r][c], -int(e))
                g = -g if det < 0 else g
                assert isinstance(g, np.float64)
                m[3 * r + c] = F(g)  # round to nearest even, denormals kept
        return m, 1


def clamp_fill(fill, u8):
    return min(max(int(fill), 0), 255) if u8 else int(fill)


def sample(m, model, source, Hd, Wd, fill):
    """Steps 2-4: (the Hd x Wd output in the source's dtype, the covered mask)."""
    source = np.asarray(source)
    u8 = source.dtype == np.uint8
    assert u8 or source.dtype == np.int32
    Hs, Ws = source.shape
    out = np.full((Hd, Wd), clamp_fill(fill, u8), source.dtype)
    if not model:
        return out, np.zeros((Hd, Wd), bool)
    m = [F(v) for v in np.asarray(m, F)]
    with np.errstate(all="ignore"):
        x = np.arange(Wd).astype(F)[None, :]
        y = np.arange(Hd).astype(F)[:, None]
        u = (m[0] * x + m[1] * y) + m[2]
        v = (m[3] * x + m[4] * y) + m[5]
        w = (m[6] * x + m[7] * y) + m[8]
        sx, sy = u / w, v / w
        for a in (u, v, w, sx, sy):
            assert a.dtype == F
        cov = (w > 0) & (sx >= 0) & (sy >= 0) & (sx <= F(Ws - 1)) & (sy <= F(Hs - 1))  # a NaN fails
        cov = np.broadcast_to(cov, (Hd, Wd))
        sx, sy = np.broadcast_to(sx, (Hd, Wd))[cov], np.broadcast_to(sy, (Hd, Wd))[cov]
        x0f, y0f = np.floor(sx), np.floor(sy)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
        fx, fy = sx - x0f, sy - y0f
        p00, p01, p10, p11 = (source[a, b].astype(F) for a, b in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
        top = p00 + fx * (p01 - p00)
        bot = p10 + fx * (p11 - p10)
        val = top + fy * (bot - top)
        q = np.rint(val)
        for a in (fx, fy, top, bot, val, q):
            assert a.dtype == F
        if u8:
            res = np.clip(q, 0, 255).astype(np.uint8)
        else:
            res = np.where(q >= F(2147483648.0), INT32_MAX, np.where(q < F(-2147483648.0), INT32_MIN,
                                                                     np.clip(q, -2147483648.0, 2147483520.0).astype(np.int64)))
        out[cov] = res.astype(source.dtype)
    return out, cov


def np_warp(h, direction, query, train, fill=0, none=False):
    """(the warped image, the 64-byte record) of the rule: `query` and `train` are the two images
    (int32 or uint8 arrays), h maps query (x, y) to train coordinates."""
    source, dest = (train, query) if direction == TRAIN_TO_QUERY else (query, train)
    dest = np.asarray(dest)
    Hd, Wd = dest.shape
    m, model = matrix(h, direction, none)
    out, cov = sample(m, model, source, Hd, Wd, fill)
    rec = np.zeros(1, WARP_DT)
    rec["m"], rec["model"], rec["pixels"], rec["direction"] = m, model, Hd * Wd, direction
    rec["covered"] = np.count_nonzero(cov)
    rec["sad"] = int(np.abs(out.astype(np.int64)[cov] - dest.astype(np.int64)[cov]).sum())  # exact integers
    return out, rec[0]


def np_warp_model(model_rec, direction, query, train, fill=0):
    """np_warp under a gdp_homography model record (HOMOGRAPHY_DT), "none" included."""
    return np_warp(model_rec["h"], direction, query, train, fill, none=int(model_rec["hypothesis"]) == NONE)


def loop_warp(h, direction, query, train, fill=0, none=False):
    """The same rule as a plain per-pixel Python loop (for small images): the vectorised form's check."""
    source, dest = (train, query) if direction == TRAIN_TO_QUERY else (query, train)
    source, dest = np.asarray(source), np.asarray(dest)
    u8 = source.dtype == np.uint8
    Hs, Ws = source.shape
    Hd, Wd = dest.shape
    m, model = matrix(h, direction, none)
    out = np.full((Hd, Wd), clamp_fill(fill, u8), source.dtype)
    covered, sad = 0, 0
    with np.errstate(all="ignore"):
        for r in range(Hd if model else 0):
            for c in range(Wd):
                x, y = F(c), F(r)
                u = (m[0] * x + m[1] * y) + m[2]
                v = (m[3] * x + m[4] * y) + m[5]
                w = (m[6] * x + m[7] * y) + m[8]
                if not w > 0:
                    continue
                sx, sy = u / w, v / w
                if not (sx >= 0 and sy >= 0 and sx <= F(Ws - 1) and sy <= F(Hs - 1)):
                    continue
                x0f, y0f = np.floor(sx), np.floor(sy)
                x0, y0 = int(x0f), int(y0f)
                x1, y1 = min(x0 + 1, Ws - 1), min(y0 + 1, Hs - 1)
                fx, fy = sx - x0f, sy - y0f
                p00, p01, p10, p11 = F(source[y0, x0]), F(source[y0, x1]), F(source[y1, x0]), F(source[y1, x1])
                top = p00 + fx * (p01 - p00)
                bot = p10 + fx * (p11 - p10)
                val = top + fy * (bot - top)
                q = np.rint(val)
                assert isinstance(q, F)
                if u8:
                    o = min(max(int(q), 0), 255)
                else:
                    o = INT32_MAX if q >= F(2147483648.0) else INT32_MIN if q < F(-2147483648.0) else int(q)
                out[r, c] = o
                covered += 1
                sad += abs(o - int(dest[r, c]))
    rec = np.zeros(1, WARP_DT)
    rec["m"], rec["model"], rec["pixels"], rec["direction"] = m, model, Hd * Wd, direction
    rec["covered"], rec["sad"] = covered, sad
    return out, rec[0]
