"""Shared by the orientation tests (a plain module, no fixtures): the numpy float32 oracle that
implements the rule of gdp_orient_keypoints (include/gdp.h) literally, one separately rounded float32
operation per operation of the rule and in its order, vectorised over the records of one (octave,
scale); and the gradient pyramids whose orientation is known in closed form.  The weight table is an
argument: glibc expf and numpy may differ in the last bit, so the GPU tests hand the LIBRARY's table
to the oracle.  tests/test_orient_oracle.py checks the oracle itself on the CPU."""
import numpy as np

from extrema_oracle import F, octave_levels, packed_size

BINS = 36
# T[k], k = 1..8: the float32 nearest to tan(k * 10 degrees), as gdp.h writes them
T_BITS = (0x3e348f0f, 0x3eba5a4e, 0x3f13cd3a, 0x3f56cf3c, 0x3f988b62, 0x3fddb3d7, 0x402fd6ac, 0x40b57b24)
T = np.array(T_BITS, np.uint32).view(np.float32)
REASONS = ("ok", "nonfinite", "flat")
ORIENTED_FIELDS = ("octave", "scale", "kind", "row", "col", "value", "dscale", "drow", "dcol", "interp", "angle", "peak",
                   "bin", "peaks")
REFINED_DT = np.dtype({"names": ["octave", "scale", "kind", "row", "col", "value", "dscale", "drow", "dcol", "interp"],
                       "formats": [np.uint16, np.uint8, np.int8, np.int32, np.int32] + [np.float32] * 5,
                       "offsets": [0, 2, 3, 4, 8, 12, 16, 20, 24, 28], "itemsize": 32})
INF = F(np.inf)


def radius(s):
    return (9 + s) // (s + 1)


def formula_weights(s):
    """w_s[d2]: the rule's float32 argument -((float)d2 * k_s), the exponential in float64 rounded to
    float32 (within 1 ulp of the library's table, whose expf is glibc's)."""
    R = radius(s)
    arg = -(np.arange(2 * R * R + 1).astype(F) * (F((s + 1) * (s + 1)) / F(18.0)))
    assert arg.dtype == np.float32
    return np.exp(arg.astype(np.float64)).astype(np.float32)


def formula_tables(S):
    return {s: formula_weights(s) for s in range(1, S + 1)}


def np_bin(gx, gy):
    """The bin of float32 arrays gx, gy: the quadrant, then the count of passed boundaries."""
    gx, gy = np.asarray(gx, F), np.asarray(gy, F)
    zero = F(0)
    q0 = (gx > zero) & (gy >= zero)
    q1 = ~q0 & (gx <= zero) & (gy > zero)
    q2 = ~q0 & ~q1 & (gx < zero) & (gy <= zero)
    q = np.where(q0, 0, np.where(q1, 1, np.where(q2, 2, 3)))
    ax = np.where(q0, gx, np.where(q1, gy, np.where(q2, -gx, -gy))).astype(F)
    ay = np.where(q0, gy, np.where(q1, -gx, np.where(q2, -gy, gx))).astype(F)
    j = np.zeros(gx.shape, np.int64)
    with np.errstate(all="ignore"):
        for k in range(8):
            prod = ax * T[k]
            assert prod.dtype == np.float32
            j += ay >= prod
    return 9 * q + j


def gaussian_level(D, S, s):
    """L = P[S+2]; for t = S+1 down to s: L = L + P[t].  Levels below s are not touched."""
    L = D[S + 2].copy()
    for t in range(S + 1, s - 1, -1):
        L = L + D[t]
    assert L.dtype == np.float32
    return L


def np_orient(packed, H, W, S, O, records, tables, clipped_out=None):
    """Orient `records` (a structured array with the fields of gdp_keypoint_refined) on the packed
    [o][s][rows][cols] pyramid with the weight tables {s: w_s}.  Returns (out, reasons): `out` the
    multiset of output records as a sorted list of tuples (octave, scale, kind, row, col, the BITS of
    value, dscale, drow, dcol, interp, angle, peak, then bin, peaks), `reasons` one of REASONS per
    input in input order: ok, nonfinite (a NaN or inf magnitude or smoothed bin), flat (no peak: an
    all-zero histogram).  clipped_out, a list, receives per input whether its window met the border."""
    assert packed.dtype == np.float32 and packed.size == packed_size(H, W, S, O)
    records = np.asarray(records)
    n = len(records)
    o_all = records["octave"].astype(np.int64)
    s_all = records["scale"].astype(np.int64)
    r_all = records["row"].astype(np.int64)
    c_all = records["col"].astype(np.int64)
    reasons = np.full(n, "", dtype=object)
    clipped = np.zeros(n, bool)
    out = []
    levels = octave_levels(packed, H, W, S, O)
    fbits = lambda a: np.ascontiguousarray(a).view(np.uint32).astype(np.int64)  # noqa: E731
    with np.errstate(all="ignore"):
        for o, s in sorted(set(zip(o_all.tolist(), s_all.tolist()))):
            idx = np.nonzero((o_all == o) & (s_all == s))[0]
            D = levels[o]
            rows, cols = D.shape[1:]
            assert 1 <= s <= S
            r, c = r_all[idx], c_all[idx]
            assert ((r >= 1) & (r <= rows - 2) & (c >= 1) & (c <= cols - 2)).all()
            L = gaussian_level(D, S, s)
            R, w = radius(s), tables[s]
            assert w.dtype == np.float32 and w.size == 2 * R * R + 1
            m_ = len(idx)
            ar = np.arange(m_)
            bad = np.zeros(m_, bool)
            hist = np.zeros((m_, BINS), F)
            for dr in range(-R, R + 1):
                part = np.zeros((m_, BINS), F)  # a skipped row stays a partial of +0
                rr = r + dr
                row_ok = (rr >= 1) & (rr <= rows - 2)
                for dc in range(-R, R + 1):
                    cc = c + dc
                    ok = row_ok & (cc >= 1) & (cc <= cols - 2)
                    clipped[idx] |= ~ok
                    ra, ca = np.where(ok, rr, 1), np.where(ok, cc, 1)  # a skipped sample reads a harmless place
                    gx = L[ra, ca + 1] - L[ra, ca - 1]
                    gy = L[ra + 1, ca] - L[ra - 1, ca]
                    mag = np.sqrt(gx * gx + gy * gy)
                    assert mag.dtype == np.float32
                    bad |= ok & ~(mag < INF)
                    add = ok & (mag < INF) & (mag > F(0))
                    b = np_bin(gx, gy)
                    term = mag * w[dr * dr + dc * dc]
                    assert term.dtype == np.float32
                    part[ar[add], b[add]] = part[ar[add], b[add]] + term[add]
                hist = hist + part
            h = ((np.roll(hist, 2, 1) + np.roll(hist, -2, 1)) * F(0.0625) +
                 (np.roll(hist, 1, 1) + np.roll(hist, -1, 1)) * F(0.25)) + hist * F(0.375)
            assert h.dtype == np.float32
            bad |= ~(np.abs(h) < INF).all(axis=1)
            mx = h[:, 0].copy()
            for k in range(1, BINS):
                mx = np.where(h[:, k] > mx, h[:, k], mx)
            thr = mx * F(0.8)
            left, right = np.roll(h, 1, 1), np.roll(h, -1, 1)
            peak = (h > left) & (h > right) & (h >= thr[:, None]) & ~bad[:, None]
            npeaks = peak.sum(axis=1)
            kk = np.broadcast_to(np.arange(BINS, dtype=np.float32), h.shape)
            bb = kk + (F(0.5) * (left - right)) / ((left - F(2) * h) + right)
            bb = np.where(bb < F(0), bb + F(36), bb)
            bb = np.where(bb >= F(36), bb - F(36), bb)
            angle = bb * F(10)
            assert angle.dtype == np.float32
            reasons[idx] = np.where(bad, "nonfinite", np.where(npeaks == 0, "flat", "ok"))
            rec = records[idx]
            for i, k in zip(*np.nonzero(peak)):
                t = rec[i]
                out.append((int(t["octave"]), int(t["scale"]), int(t["kind"]), int(t["row"]), int(t["col"])) +
                           tuple(int(fbits(rec[f][i:i + 1])[0]) for f in ("value", "dscale", "drow", "dcol", "interp")) +
                           (int(fbits(angle[i, k:k + 1])[0]), int(fbits(h[i, k:k + 1])[0]), int(k), int(npeaks[i])))
    assert all(x in REASONS for x in reasons)
    if clipped_out is not None:
        clipped_out[:] = clipped.tolist()
    return sorted(out), reasons.tolist()


def as_multiset(oriented):
    """The sorted tuples np_orient returns, from an ORIENTED_DTYPE array."""
    a = np.asarray(oriented)
    cols = [a[f].astype(np.int64).tolist() for f in ORIENTED_FIELDS[:5]]
    cols += [np.ascontiguousarray(a[f]).view(np.uint32).tolist() for f in ORIENTED_FIELDS[5:12]]
    cols += [a[f].astype(np.int64).tolist() for f in ORIENTED_FIELDS[12:]]
    return sorted(zip(*cols))


def assert_download_order(oriented):
    """gdp_download_oriented's order: (octave, scale, row, col, bin), ties by the twelve words."""
    a = np.ascontiguousarray(oriented)
    words = a.view(np.uint32).reshape(len(a), 12)
    keys = [(int(t["octave"]), int(t["scale"]), int(t["row"]), int(t["col"]), int(t["bin"])) + tuple(w.tolist())
            for t, w in zip(a, words)]
    assert keys == sorted(keys)


def refined_records(points, octave=0, kind=1, offsets=(0.25, -0.125, 0.5), value=1.5, interp=2.5):
    """A refined record array from (scale, row, col) triples; the float fields are copied through by
    the orientation, so they carry recognisable values."""
    out = np.zeros(len(points), REFINED_DT)
    for k, (s, r, c) in enumerate(points):
        out[k] = (octave, s, kind, r, c, value, offsets[0], offsets[1], offsets[2], interp)
    return out


def refined_from(kp):
    """Refined records at the samples of a keypoint record array (value kept, offsets zero)."""
    kp = np.asarray(kp)
    out = np.zeros(len(kp), REFINED_DT)
    for f in ("octave", "scale", "kind", "row", "col", "value"):
        out[f] = kp[f]
    return out


# ---------------------------------------------------------------------------------------------
# gradient pyramids: the orientation in closed form
# ---------------------------------------------------------------------------------------------
DIRECTIONS = (((1, 0), 0), ((0, 1), 9), ((-1, 0), 18), ((0, -1), 27), ((1, 1), 4), ((-1, 1), 13), ((-1, -1), 22), ((1, -1), 31))


def gradient_pyramid(S, rows, cols, s, a, b):
    """One octave [S+3][rows][cols]: level S+2 = a * col, level S+1 = b * row, levels s..S zero and
    the levels below s NaN — a read below s rejects everything.  L = a * col + b * row exactly, so
    every sample has (gx, gy) = (2a, 2b): one bin, one peak, angle = 10 * bin exactly."""
    D = np.zeros((S + 3, rows, cols), F)
    D[:s] = np.nan
    D[S + 2] = F(a) * np.arange(cols, dtype=F)[None, :]
    D[S + 1] = F(b) * np.arange(rows, dtype=F)[:, None]
    return D
