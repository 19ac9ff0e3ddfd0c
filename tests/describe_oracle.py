"""Shared by the descriptor tests (a plain module, no fixtures): the numpy float32 oracle that
implements the rule of gdp_describe_keypoints (include/gdp.h) literally, one separately rounded
float32 operation per operation of the rule and in its order, vectorised over the records of one
(octave, scale); the formulas of its tables; and a float64 SIFT descriptor with real cos, sin, atan2
and exp to hold the rule against.  The weight and rotation tables are arguments: glibc expf and numpy
may differ in the last bit, so the GPU tests hand the LIBRARY's tables to the oracle.
tests/test_describe_oracle.py checks the oracle itself on the CPU."""
import math

import numpy as np

from extrema_oracle import F, octave_levels, packed_size
from orient_oracle import ORIENTED_FIELDS, gaussian_level

BINS = 128
ANGLES = 1440
A_BITS = (0x3fa2f890, 0xbed8d61d, 0x3e7c5661, 0xbe17cbe9, 0x3d89486e, 0xbc74784e)  # c0..c5, as gdp.h writes them
A_COEF = np.array(A_BITS, np.uint32).view(np.float32)
REASONS = ("ok", "dropped", "nonfinite", "flat")
ORIENTED_DT = np.dtype({"names": list(ORIENTED_FIELDS),
                        "formats": [np.uint16, np.uint8, np.int8, np.int32, np.int32] + [np.float32] * 7 + [np.uint32] * 2,
                        "offsets": [0, 2, 3, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44], "itemsize": 48})
INF = F(np.inf)


def radius(s):
    return (2121 + 50 * (s + 1)) // (100 * (s + 1))


def formula_weights(s):
    """W_s[d2]: the rule's float32 argument -((float)d2 * k_s), the exponential in float64 rounded to
    float32 (within 1 ulp of the library's table, whose expf is glibc's)."""
    R = radius(s)
    arg = -(np.arange(2 * R * R + 1).astype(F) * (F((s + 1) * (s + 1)) / F(288.0)))
    assert arg.dtype == np.float32
    return np.exp(arg.astype(np.float64)).astype(np.float32)


def formula_rotation():
    """(C, S): Q[m] = (float)cos(m pi / 720) in double over the first quadrant, Q[0] = 1 and Q[360] = 0
    exactly, turned through the other three quadrants by (c, s) -> (-s, c)."""
    Q = np.array([math.cos(m * math.pi / 720.0) for m in range(361)]).astype(np.float32)
    Q[0], Q[360] = 1.0, 0.0
    C, S = np.zeros(ANGLES, F), np.zeros(ANGLES, F)
    for a in range(ANGLES):
        k, m = divmod(a, 360)
        c, s = Q[m], Q[360 - m]
        for _ in range(k):
            c, s = -s, c
        C[a], S[a] = c, s
    return C, S


def formula_tables(S):
    """({s: W_s}, C, S) from the formulas: what the CPU tests feed the oracle."""
    return ({s: formula_weights(s) for s in range(1, S + 1)},) + formula_rotation()


def np_octant(t):
    """A(t) ~ atan(t) 4 / pi on [0, 1] for a float32 array: Horner, every * and + rounded."""
    t = np.asarray(t, F)
    z = t * t
    p = np.full(t.shape, A_COEF[5], F)
    for k in range(4, -1, -1):
        p = p * z + A_COEF[k]
        assert p.dtype == np.float32
    return p * t


def np_orientation(gu, gv):
    """ob in [0, 8) of float32 arrays (gu, gv): the quadrant, then the polynomial."""
    gu, gv = np.asarray(gu, F), np.asarray(gv, F)
    zero = F(0)
    q0 = (gu > zero) & (gv >= zero)
    q1 = ~q0 & (gu <= zero) & (gv > zero)
    q2 = ~q0 & ~q1 & (gu < zero) & (gv <= zero)
    q = np.where(q0, 0, np.where(q1, 1, np.where(q2, 2, 3)))
    ax = np.where(q0, gu, np.where(q1, gv, np.where(q2, -gu, -gv))).astype(F)
    ay = np.where(q0, gv, np.where(q1, -gu, np.where(q2, -gv, gu))).astype(F)
    with np.errstate(all="ignore"):
        low = ay <= ax
        w_low = np.where(ax > zero, np_octant(np.where(low & (ax > zero), ay / ax, zero)), zero)
        w_high = F(2.0) - np_octant(np.where(low, zero, ax / ay))
        w8 = np.where(low, w_low, w_high).astype(F)
        ob = (2 * q).astype(F) + w8
        ob = np.where(ob >= F(8.0), ob - F(8.0), ob)
    assert ob.dtype == np.float32
    return ob


def tree_sum_squares(v):
    """T(v) over the last axis of a float32 [n][128] array."""
    t = v * v
    step = BINS // 2
    while step >= 1:
        t = t[:, :step] + t[:, step:2 * step]
        step //= 2
    assert t.dtype == np.float32 and t.shape[1] == 1
    return t[:, 0]


def np_describe(packed, H, W, S, O, records, weights, cosv, sinv, clipped_out=None):
    """Describe `records` (a structured array with the fields of gdp_keypoint_oriented) on the packed
    [o][s][rows][cols] pyramid with the weight tables {s: W_s} and the rotation table (cosv, sinv).
    Returns (out, reasons): `out` the multiset of output records as a sorted list of tuples (octave,
    scale, kind, row, col, the BITS of value, dscale, drow, dcol, interp, angle, peak, then bin, peaks,
    then the 128 descriptor bytes as a tuple), `reasons` one of REASONS per input in input order.
    clipped_out, a list, receives per input whether its window met the border."""
    assert packed.dtype == np.float32 and packed.size == packed_size(H, W, S, O)
    assert cosv.dtype == np.float32 and sinv.dtype == np.float32 and cosv.size == ANGLES and sinv.size == ANGLES
    records = np.asarray(records)
    n = len(records)
    levels = octave_levels(packed, H, W, S, O)
    o_all = records["octave"].astype(np.int64)
    s_all = records["scale"].astype(np.int64)
    r_all = records["row"].astype(np.int64)
    c_all = records["col"].astype(np.int64)
    ang_all = records["angle"].astype(F)
    reasons = np.full(n, "dropped", dtype=object)
    clipped = np.zeros(n, bool)
    desc_all = np.zeros((n, BINS), np.uint8)
    # the drop test, before anything is read
    valid = np.zeros(n, bool)
    for i in range(n):
        if o_all[i] < O and 1 <= s_all[i] <= S:
            rows, cols = levels[o_all[i]].shape[1:]
            valid[i] = (1 <= r_all[i] <= rows - 2 and 1 <= c_all[i] <= cols - 2 and
                        bool(F(0.0) <= ang_all[i]) and bool(ang_all[i] < F(360.0)))
    with np.errstate(all="ignore"):
        for o, s in sorted(set(zip(o_all[valid].tolist(), s_all[valid].tolist()))):
            idx = np.nonzero(valid & (o_all == o) & (s_all == s))[0]
            D = levels[o]
            rows, cols = D.shape[1:]
            r, c = r_all[idx], c_all[idx]
            L = gaussian_level(D, S, s)
            R, w = radius(s), weights[s]
            assert w.dtype == np.float32 and w.size == 2 * R * R + 1
            inv_s = F(s + 1) / F(6.0)
            a = (ang_all[idx] * F(4.0) + F(0.5)).astype(np.int64)
            a = np.where(a >= ANGLES, a - ANGLES, a)
            ca, sa = cosv[a], sinv[a]
            m_ = len(idx)
            ar = np.arange(m_)
            bad = np.zeros(m_, bool)
            hist = np.zeros((m_, BINS), F)
            for dr in range(-R, R + 1):
                part = np.zeros((m_, BINS), F)  # a skipped row stays a partial of +0
                rr = r + dr
                row_ok = (rr >= 1) & (rr <= rows - 2)
                y = F(dr)
                for dc in range(-R, R + 1):
                    cc = c + dc
                    inside = row_ok & (cc >= 1) & (cc <= cols - 2)
                    clipped[idx] |= ~inside
                    x = F(dc)
                    cb = ((x * ca + y * sa) * inv_s) + F(1.5)
                    rb = ((y * ca - x * sa) * inv_s) + F(1.5)
                    assert cb.dtype == np.float32 and rb.dtype == np.float32
                    ok = inside & (rb > F(-1)) & (rb < F(4)) & (cb > F(-1)) & (cb < F(4))
                    if not ok.any():
                        continue
                    ra, cx = np.where(ok, rr, 1), np.where(ok, cc, 1)  # a skipped sample reads a harmless place
                    gx = L[ra, cx + 1] - L[ra, cx - 1]
                    gy = L[ra + 1, cx] - L[ra - 1, cx]
                    mag = np.sqrt(gx * gx + gy * gy)
                    assert mag.dtype == np.float32
                    bad |= ok & ~(mag < INF)
                    add = ok & (mag < INF) & (mag > F(0))
                    gu = gx * ca + gy * sa
                    gv = gy * ca - gx * sa
                    ob = np_orientation(np.where(add, gu, F(1)), np.where(add, gv, F(0)))
                    r0, c0, o0 = np.floor(rb), np.floor(cb), np.floor(ob)
                    fr, fc, fo = rb - r0, cb - c0, ob - o0
                    val = mag * w[dr * dr + dc * dc]
                    assert val.dtype == np.float32 and fr.dtype == np.float32
                    ir, ic, io = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
                    v1 = val * fr
                    v0 = val - v1
                    for i, v in ((0, v0), (1, v1)):
                        vc1 = v * fc
                        vc0 = v - vc1
                        for j, vc in ((0, vc0), (1, vc1)):
                            vo1 = vc * fo
                            vo0 = vc - vo1
                            for k, vo in ((0, vo0), (1, vo1)):
                                br, bc = ir + i, ic + j
                                put = add & (br >= 0) & (br <= 3) & (bc >= 0) & (bc <= 3)
                                b = ((br * 4 + bc) * 8 + ((io + k) % 8))[put]
                                assert vo.dtype == np.float32
                                part[ar[put], b] = part[ar[put], b] + vo[put]
                hist = hist + part
            bad |= ~(hist < INF).all(axis=1)
            n1 = np.sqrt(tree_sum_squares(hist))
            keep = ~bad & (n1 > F(0)) & (n1 < INF)
            h = hist / n1[:, None]
            h = np.where(h > F(0.2), F(0.2), h)
            n2 = np.sqrt(tree_sum_squares(h))
            qv = (h / n2[:, None]) * F(512.0)
            assert qv.dtype == np.float32
            safe = np.where(keep[:, None] & (qv < F(255.0)), qv, F(0))
            desc = np.where(qv >= F(255.0), 255, safe.astype(np.int64)).astype(np.uint8)
            desc_all[idx] = desc
            reasons[idx] = np.where(bad, "nonfinite", np.where(keep, "ok", "flat"))
    assert all(x in REASONS for x in reasons)
    if clipped_out is not None:
        clipped_out[:] = clipped.tolist()
    out = [record_tuple(records[i], desc_all[i]) for i in range(n) if reasons[i] == "ok"]
    return sorted(out), reasons.tolist()


def record_tuple(t, desc):
    fbits = lambda f: int(np.array([t[f]], np.float32).view(np.uint32)[0])  # noqa: E731
    return ((int(t["octave"]), int(t["scale"]), int(t["kind"]), int(t["row"]), int(t["col"])) +
            tuple(fbits(f) for f in ORIENTED_FIELDS[5:12]) + (int(t["bin"]), int(t["peaks"]), tuple(int(x) for x in desc)))


def as_multiset(described):
    """The sorted tuples np_describe returns, from a DESCRIBED_DTYPE array."""
    a = np.asarray(described)
    return sorted(record_tuple(t, t["desc"]) for t in a)


def assert_download_order(described):
    """gdp_download_described's order: (octave, scale, row, col, bin), ties by the 44 words."""
    a = np.ascontiguousarray(described)
    words = a.view(np.uint32).reshape(len(a), 44)
    keys = [(int(t["octave"]), int(t["scale"]), int(t["row"]), int(t["col"]), int(t["bin"])) + tuple(w.tolist())
            for t, w in zip(a, words)]
    assert keys == sorted(keys)


def oriented_records(points, octave=0, kind=1, offsets=(0.25, -0.125, 0.5), value=1.5, interp=2.5, peak=3.5):
    """An oriented record array from (scale, row, col, angle) tuples; the other fields are copied
    through by the description, so they carry recognisable values."""
    out = np.zeros(len(points), ORIENTED_DT)
    for k, (s, r, c, angle) in enumerate(points):
        out[k] = (octave, s, kind, r, c, value, offsets[0], offsets[1], offsets[2], interp, angle, peak, k % 36, 1)
    return out


# ---------------------------------------------------------------------------------------------
# the float64 descriptor the rule is held against
# ---------------------------------------------------------------------------------------------
def float64_descriptor(L, s, r, c, angle):
    """Lowe's descriptor of sample (r, c) of the Gaussian level L (float64 arithmetic, real cos, sin,
    atan2 and exp, the unquantised angle, plain sums): the same window, bin width, weighting, split,
    clipping and quantisation as the rule.  Returns 128 bytes, or None for a flat window."""
    L = L.astype(np.float64)
    rows, cols = L.shape
    R = radius(s)
    inv = (s + 1) / 6.0
    k = (s + 1) * (s + 1) / 288.0
    ca, sa = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    hist = np.zeros((4, 4, 8))
    for dr in range(-R, R + 1):
        for dc in range(-R, R + 1):
            rr, cc = r + dr, c + dc
            if not (1 <= rr <= rows - 2 and 1 <= cc <= cols - 2):
                continue
            cb = (dc * ca + dr * sa) * inv + 1.5
            rb = (dr * ca - dc * sa) * inv + 1.5
            if not (-1 < rb < 4 and -1 < cb < 4):
                continue
            gx = L[rr, cc + 1] - L[rr, cc - 1]
            gy = L[rr + 1, cc] - L[rr - 1, cc]
            m = math.hypot(gx, gy)
            if not m > 0:
                continue
            ob = ((math.degrees(math.atan2(gy, gx)) - angle) % 360.0) / 45.0
            if ob >= 8.0:
                ob -= 8.0
            r0, c0, o0 = math.floor(rb), math.floor(cb), math.floor(ob)
            fr, fc, fo = rb - r0, cb - c0, ob - o0
            mag = m * math.exp(-(dr * dr + dc * dc) * k)
            for i, wr in ((0, 1 - fr), (1, fr)):
                for j, wc in ((0, 1 - fc), (1, fc)):
                    if 0 <= r0 + i <= 3 and 0 <= c0 + j <= 3:
                        for t, wo in ((0, 1 - fo), (1, fo)):
                            hist[r0 + i, c0 + j, (o0 + t) % 8] += mag * wr * wc * wo
    v = hist.ravel()
    n = math.sqrt((v * v).sum())
    if not n > 0:
        return None
    v = np.minimum(v / n, 0.2)
    v = v / math.sqrt((v * v).sum()) * 512.0
    return np.where(v >= 255.0, 255, v.astype(np.int64)).astype(np.uint8)
