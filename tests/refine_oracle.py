"""Shared by the refinement tests (a plain module, no fixtures): the numpy float32 oracle that
implements the rule of gdp_refine_keypoints (include/gdp.h) literally, one separately rounded float32
operation per operation of the rule, and the quadratic pyramids whose refinement is known in closed
form.  tests/test_refine_oracle.py checks the oracle itself on the CPU."""
import functools

import numpy as np

from extrema_oracle import F, packed_size, want

MAX_STEPS = 5  # GDP_REFINE_MAX_STEPS
REASONS = ("ok", "singular", "nan", "left", "steps", "contrast", "edge")
REFINED_FIELDS = ("octave", "scale", "kind", "row", "col", "value", "dscale", "drow", "dcol", "interp")


def _f32(*arrays):
    for a in arrays:
        assert a.dtype == np.float32, a.dtype


def np_refine(packed, H, W, S, O, records, contrast=0.0, edge_ratio=0.0, moves_out=None):
    """Refine `records` (any structured array with octave, scale, kind, row, col) on the packed
    [o][s][rows][cols] pyramid.  Returns (kept, reasons): `kept` the multiset of kept records as a
    sorted list of tuples (octave, scale, kind, row, col, then the BITS of value, dscale, drow, dcol,
    interp), `reasons` one of REASONS for every input, in input order: ok (kept), singular (det zero
    or NaN), nan (a NaN offset: nothing moved), left (walked out of the candidates), steps (no
    convergence in MAX_STEPS solves), contrast (|interp| not above the threshold, NaN included), edge.
    moves_out, a list, receives the number of moves of every input."""
    assert packed.dtype == np.float32 and packed.size == packed_size(H, W, S, O)
    records = np.asarray(records)
    n = len(records)
    o = records["octave"].astype(np.int64)
    s = records["scale"].astype(np.int64)
    r = records["row"].astype(np.int64)
    c = records["col"].astype(np.int64)
    assert n == 0 or (o.max() < O and s.min() >= 1 and s.max() <= S)
    rows_o = np.array([H >> k for k in range(O)], np.int64)
    cols_o = np.array([W >> k for k in range(O)], np.int64)
    off_o = np.concatenate(([0], np.cumsum((S + 3) * rows_o * cols_o)[:-1])).astype(np.int64)
    rows, cols, off = rows_o[o], cols_o[o], off_o[o]
    assert n == 0 or ((r >= 1) & (r <= rows - 2) & (c >= 1) & (c <= cols - 2)).all()
    lev = rows * cols

    reason = np.full(n, "", dtype=object)
    moves = np.zeros(n, np.int64)
    out = {k: np.zeros(n, np.float32) for k in ("v", "xs", "xr", "xc", "interp", "hcc", "hrr", "hrc")}
    active = np.ones(n, bool)
    half, quarter, two = F(0.5), F(0.25), F(2)
    with np.errstate(all="ignore"):
        for _ in range(MAX_STEPS):
            idx = np.nonzero(active)[0]
            if idx.size == 0:
                break
            q = off[idx] + s[idx] * lev[idx] + r[idx] * cols[idx] + c[idx]
            dC, dR, dS = 1, cols[idx], lev[idx]
            D = lambda d: packed[q + d]  # noqa: E731  (level S+2 is never reached: s <= S)
            v = D(0)
            gc = (D(dC) - D(-dC)) * half
            gr = (D(dR) - D(-dR)) * half
            gs = (D(dS) - D(-dS)) * half
            hcc = (D(dC) + D(-dC)) - two * v
            hrr = (D(dR) + D(-dR)) - two * v
            hss = (D(dS) + D(-dS)) - two * v
            hrc = ((D(dR + dC) - D(dR - dC)) - (D(-dR + dC) - D(-dR - dC))) * quarter
            hsc = ((D(dS + dC) - D(dS - dC)) - (D(-dS + dC) - D(-dS - dC))) * quarter
            hsr = ((D(dS + dR) - D(dS - dR)) - (D(-dS + dR) - D(-dS - dR))) * quarter
            A = hrr * hss - hsr * hsr
            B = hrc * hss - hsc * hsr
            C = hrc * hsr - hsc * hrr
            E = hcc * hss - hsc * hsc
            Q = hcc * hsr - hrc * hsc
            G = hcc * hrr - hrc * hrc
            det = (hcc * A - hrc * B) + hsc * C
            xc = -(((A * gc - B * gr) + C * gs) / det)
            xr = -(((E * gr - B * gc) - Q * gs) / det)
            xs = -(((C * gc - Q * gr) + G * gs) / det)
            interp = v + ((gc * xc + gr * xr) + gs * xs) * half
            _f32(v, gc, gr, gs, hcc, hrr, hss, hrc, hsc, hsr, A, B, C, E, Q, G, det, xc, xr, xs, interp)

            solvable = np.abs(det) > F(0)
            reason[idx[~solvable]] = "singular"  # det is zero or NaN
            conv = solvable & (np.abs(xc) <= half) & (np.abs(xr) <= half) & (np.abs(xs) <= half)
            for k, a in (("v", v), ("xs", xs), ("xr", xr), ("xc", xc), ("interp", interp), ("hcc", hcc), ("hrr", hrr),
                         ("hrc", hrc)):
                out[k][idx[conv]] = a[conv]
            reason[idx[conv]] = "ok"
            go = solvable & ~conv
            mc = (xc > half).astype(np.int64) - (xc < -half).astype(np.int64)
            mr = (xr > half).astype(np.int64) - (xr < -half).astype(np.int64)
            ms = (xs > half).astype(np.int64) - (xs < -half).astype(np.int64)
            stuck = go & (mc == 0) & (mr == 0) & (ms == 0)
            reason[idx[stuck]] = "nan"
            go &= ~stuck
            g = idx[go]
            c[g] += mc[go]
            r[g] += mr[go]
            s[g] += ms[go]
            moves[g] += 1
            inside = (s[g] >= 1) & (s[g] <= S) & (r[g] >= 1) & (r[g] <= rows[g] - 2) & (c[g] >= 1) & (c[g] <= cols[g] - 2)
            reason[g[~inside]] = "left"
            active[:] = False
            active[g[inside]] = True
        reason[active] = "steps"

        ok = reason == "ok"
        passes = np.abs(out["interp"]) > F(contrast)  # a NaN fails
        reason[ok & ~passes] = "contrast"
        if edge_ratio != 0:
            er = F(edge_ratio)
            dxx, dyy, dxy = out["hcc"], out["hrr"], out["hrc"]
            tr = dxx + dyy
            det2 = dxx * dyy - dxy * dxy
            _f32(tr, det2)
            edge_ok = (det2 > F(0)) & ((tr * tr) * er < ((er + F(1)) * (er + F(1))) * det2)
            reason[(reason == "ok") & ~edge_ok] = "edge"
    assert all(x in REASONS for x in reason)
    if moves_out is not None:
        moves_out[:] = moves.tolist()
    k = np.nonzero(reason == "ok")[0]
    bits = lambda a: a[k].view(np.uint32).tolist()  # noqa: E731
    kept = sorted(zip(o[k].tolist(), s[k].tolist(), records["kind"][k].astype(np.int64).tolist(), r[k].tolist(), c[k].tolist(),
                      bits(out["v"]), bits(out["xs"]), bits(out["xr"]), bits(out["xc"]), bits(out["interp"])))
    return kept, reason.tolist()


def as_multiset(refined):
    """The sorted tuples np_refine returns, from a REFINED_DTYPE array."""
    a = np.asarray(refined)
    cols = [a[f].astype(np.int64).tolist() for f in REFINED_FIELDS[:5]]
    cols += [np.ascontiguousarray(a[f]).view(np.uint32).tolist() for f in REFINED_FIELDS[5:]]
    return sorted(zip(*cols))


def download_key(t):
    """gdp_download_refined's order of an as_multiset tuple: (octave, scale, row, col), then the bits
    of (dscale, drow, dcol, interp, value, kind)."""
    o, s, kind, r, c, v, xs, xr, xc, interp = t
    return (o, s, r, c, xs, xr, xc, interp, v, kind & 0xFF)


def assert_download_order(refined):
    a = np.asarray(refined)
    raw = list(zip(*([a[f].astype(np.int64).tolist() for f in REFINED_FIELDS[:5]] +
                     [np.ascontiguousarray(a[f]).view(np.uint32).tolist() for f in REFINED_FIELDS[5:]])))
    keys = [download_key(t) for t in raw]
    assert keys == sorted(keys)


def records(points, octave=0, kind=1):
    """A keypoint record array (the fields of gdp_keypoint) from (scale, row, col) triples."""
    dt = np.dtype({"names": ["octave", "scale", "kind", "row", "col", "value"],
                   "formats": [np.uint16, np.uint8, np.int8, np.int32, np.int32, np.float32],
                   "offsets": [0, 2, 3, 4, 8, 12], "itemsize": 16})
    out = np.zeros(len(points), dt)
    for k, (s, r, c) in enumerate(points):
        out[k] = (octave, s, kind, r, c, 0.0)
    return out


def records_from_set(found):
    """An np_extrema set as a record array in the order of gdp_download_keypoints."""
    rec = records([(0, 0, 0)] * len(found))
    for k, (o, s, kd, r, c, bits) in enumerate(sorted(found, key=lambda t: (t[0], t[1], t[3], t[4]))):
        rec[k] = (o, s, kd, r, c, 0.0)
        rec["value"][k:k + 1].view(np.uint32)[0] = bits
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def extrema_records(kind, shape, contrast=0.0, edge_ratio=0.0):
    """The oracle's extrema (extrema_oracle.want) of a shared pyramid as a record array."""
    return records_from_set(want(kind, shape, contrast, edge_ratio)[0])


# ---------------------------------------------------------------------------------------------
# quadratic pyramids: the refinement in closed form
# ---------------------------------------------------------------------------------------------
def quad_pyramid(S, rows, cols, s0, r0, c0, a=.5, b=.25, e=1, K=64, mix=0):
    """One octave [S+3][rows][cols] of K - a(c-c0)^2 - b(r-r0)^2 - e(s-s0)^2 + mix(c-c0)(r-r0).  With
    dyadic centres and coefficients every value, and every step of the rule on it, is exact in
    float32; the values are asserted against float64 here."""
    s, r, c = np.meshgrid(np.arange(S + 3, dtype=np.float64), np.arange(rows, dtype=np.float64),
                          np.arange(cols, dtype=np.float64), indexing="ij")
    exact = K - a * (c - c0) ** 2 - b * (r - r0) ** 2 - e * (s - s0) ** 2 + mix * (c - c0) * (r - r0)
    D = exact.astype(np.float32)
    assert np.array_equal(D.astype(np.float64), exact), "not exact in float32: use dyadic centres"
    return D


def quad_expect(start, s0, r0, c0, S, rows, cols):
    """Closed form for a quad_pyramid with mix = 0: the walk from `start` = (s, r, c) moves one sample
    per axis and step towards the centre while the distance exceeds 0.5.  Returns (final (s, r, c),
    (ds, dr, dc), moves), or None when it needs more than MAX_STEPS solves or leaves the candidates."""
    p, centre = list(start), (s0, r0, c0)
    hi = (S, rows - 2, cols - 2)
    for solve in range(MAX_STEPS):
        x = [centre[k] - p[k] for k in range(3)]
        if all(abs(v) <= 0.5 for v in x):
            return tuple(p), tuple(x), solve
        for k in range(3):
            p[k] += (x[k] > 0.5) - (x[k] < -0.5)
        if not all(1 <= p[k] <= hi[k] for k in range(3)):
            return None
    return None
