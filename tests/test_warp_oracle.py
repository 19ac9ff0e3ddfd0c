"""The numpy oracle of the warp rule (tests/warp_oracle.py) against a per-pixel loop of the same rule
and against cases whose answer is known without it.  CPU only."""
import numpy as np
import pytest

import warp_oracle as wo

F = np.float32
IDENTITY = np.eye(3, dtype=F)


def lcg(h, w, seed, dtype=np.int32, bits=8):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << bits, (h, w)).astype(dtype)


def shift(dx, dy):
    """h taking query (x, y) to train (x + dx, y + dy)."""
    return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], F)


def same(a, b):
    return a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


ROTATION = np.array([[0.92, -0.31, 2.5], [0.28, 0.95, -1.25], [1e-3, -2e-3, 1.0]], F)


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("dtype", [np.int32, np.uint8])
@pytest.mark.parametrize("h", [IDENTITY, shift(0.5, 0.25), ROTATION, np.array([[1, 0, 0], [0, 1, 0], [0.2, 0, -1]], F)],
                         ids=["identity", "half", "rotation", "w_crosses"])
def test_vectorised_equals_loop(direction, dtype, h):
    train, query = lcg(9, 11, 1, dtype), lcg(7, 10, 2, dtype)
    got, want = wo.np_warp(h, direction, query, train, fill=-3), wo.loop_warp(h, direction, query, train, fill=-3)
    assert same(got, want)
    assert got[0].shape == (query.shape if direction == 0 else train.shape)
    assert int(got[1]["pixels"]) == got[0].size and int(got[1]["direction"]) == direction and int(got[1]["reserved"]) == 0


@pytest.mark.parametrize("direction", [0, 1])
def test_identity_copies(direction):
    img = lcg(9, 11, 3)
    out, rec = wo.np_warp(IDENTITY, direction, img, img, fill=-1)
    assert np.array_equal(out, img)
    assert int(rec["covered"]) == img.size and int(rec["sad"]) == 0 and int(rec["model"]) == 1
    # direction 1: adj(I) = I scaled to 0.5 (frexp of 1 is 0.5 * 2^1)
    assert np.array_equal(rec["m"], (IDENTITY * F(0.5 if direction else 1.0)).reshape(9))


def test_integer_translation_shifts():
    train, query = lcg(9, 11, 4), lcg(9, 11, 5)
    out, rec = wo.np_warp(shift(3, 2), 0, query, train, fill=-7)
    assert np.array_equal(out[:7, :8], train[2:, 3:])  # out(r, c) = train(r + 2, c + 3)
    assert np.all(out[7:, :] == -7) and np.all(out[:, 8:] == -7)
    assert int(rec["covered"]) == 7 * 8
    assert int(rec["sad"]) == int(np.abs(train[2:, 3:].astype(np.int64) - query[:7, :8]).sum())
    back, rec1 = wo.np_warp(shift(3, 2), 1, query, train, fill=-7)  # out(r, c) = query(r - 2, c - 3)
    assert np.array_equal(back[2:, 3:], query[:7, :8]) and int(rec1["covered"]) == 7 * 8


def test_half_pixel_ties_to_even():
    ramp = np.tile(np.arange(11, dtype=np.int32), (9, 1))  # value = column
    out, rec = wo.np_warp(shift(0.5, 0), 0, ramp, ramp)
    # c + 0.5 -> 0.5, 1.5, 2.5, 3.5, ...: ties to even
    assert out[0, :10].tolist() == [0, 2, 2, 4, 4, 6, 6, 8, 8, 10]
    assert out[0, 10] == 0 and int(rec["covered"]) == 9 * 10  # sx = 10.5 > Ws - 1


def test_int32_extremes_clamp():
    yy, xx = np.indices((9, 11))
    board = np.where((yy + xx) % 2 == 0, wo.INT32_MIN, wo.INT32_MAX).astype(np.int32)
    out, rec = wo.np_warp(IDENTITY, 0, board, board)
    assert np.array_equal(out, board)  # (float)INT32_MAX = 2^31 clamps back
    assert int(rec["sad"]) == 0
    half, _ = wo.np_warp(shift(0.5, 0), 0, board, board)
    assert set(np.unique(half[:, :10]).tolist()) <= {wo.INT32_MIN, wo.INT32_MAX, 0}
    zeros = np.zeros((9, 11), np.int32)
    _, rec = wo.np_warp(IDENTITY, 0, zeros, board)
    assert int(rec["sad"]) == int(np.abs(board.astype(np.int64)).sum())  # beyond 32 bits: a uint64 sum


def test_uint8_fill_clamps():
    img = lcg(9, 11, 6, np.uint8)
    for fill, want in ((-5, 0), (300, 255), (17, 17)):
        out, rec = wo.np_warp(shift(100, 0), 0, img, img, fill=fill)
        assert out.dtype == np.uint8 and np.all(out == want) and int(rec["covered"]) == 0 and int(rec["model"]) == 1


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("k", [0, 2, 4, 8])
def test_nan_inf_never_raise(direction, bad, k):
    h = ROTATION.copy().reshape(9)
    h[k] = bad
    train, query = lcg(9, 11, 7), lcg(7, 10, 8)
    got, want = wo.np_warp(h, direction, query, train, fill=5), wo.loop_warp(h, direction, query, train, fill=5)
    assert same(got, want)
    if np.isnan(bad):  # a NaN entry reaches u, v or w of every pixel with x, y > 0, or the adjugate
        assert np.all(got[0][1:, 1:] == 5)


def test_all_nan_is_all_fill():
    img = lcg(9, 11, 9)
    out, rec = wo.np_warp(np.full(9, np.nan, F), 0, img, img, fill=9)
    assert np.all(out == 9) and int(rec["covered"]) == 0 and int(rec["model"]) == 1  # direction 0: a model, whatever the bytes
    out, rec = wo.np_warp(np.full(9, np.nan, F), 1, img, img, fill=9)
    assert np.all(out == 9) and int(rec["model"]) == 0 and not rec["m"].any()


def test_singular_has_no_model_in_direction_1():
    h = np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1]], F)  # rank 2: det = 0 exactly
    img = lcg(9, 11, 10)
    out, rec = wo.np_warp(h, 1, img, img, fill=4)
    assert int(rec["model"]) == 0 and not rec["m"].any() and np.all(out == 4) and int(rec["covered"]) == 0 and int(rec["sad"]) == 0
    _, rec0 = wo.np_warp(h, 0, img, img, fill=4)
    assert int(rec0["model"]) == 1
    out, rec = wo.np_warp(np.zeros(9, F), 1, img, img, fill=4)  # s = 0
    assert int(rec["model"]) == 0 and np.all(out == 4)


def test_none_record_is_all_fill():
    img = lcg(9, 11, 11)
    for direction in (0, 1):
        out, rec = wo.np_warp(ROTATION, direction, img, img, fill=-2, none=True)
        assert np.all(out == -2) and int(rec["model"]) == 0 and not rec["m"].any()
        assert int(rec["covered"]) == 0 and int(rec["sad"]) == 0 and int(rec["pixels"]) == img.size


def test_negative_determinant_sign_rule():
    """A mirrored, slightly rotated model with perspective (det < 0): direction 1 is direction 0 of the
    explicitly inverted matrix to within one grey level on interior pixels of a smooth image."""
    Hq, Wq, Ht, Wt = 24, 32, 28, 36
    h = np.array([[-0.98, 0.05, 33.0], [0.04, 0.97, 1.5], [2e-4, -1e-4, 1.0]], F)
    assert np.linalg.det(h.astype(np.float64)) < 0
    yy, xx = np.indices((Hq, Wq))
    query = (3 * xx + 2 * yy + 20 * np.sin(xx / 5.0) * np.cos(yy / 7.0) + 60).astype(np.int32)
    train = np.zeros((Ht, Wt), np.int32)
    got, rec = wo.np_warp(h, 1, query, train, fill=-1)
    inv = np.linalg.inv(h.astype(np.float64))
    inv = (inv / np.abs(inv).max()).astype(F)
    # direction 0 with the roles exchanged: `inv` maps train (x, y) to query coordinates
    want, rec0 = wo.np_warp(inv, 0, train, query, fill=-1)
    assert int(rec["model"]) == 1 and rec["m"][8] > 0
    both = (got != -1) & (want != -1)
    interior = np.zeros_like(both)
    interior[2:-2, 2:-2] = True
    # interior of the covered region too: a pixel whose pre-image is within a pixel of the query's edge may be
    # covered under one matrix and not under the other
    edge = np.zeros_like(both)
    edge[1:-1, 1:-1] = both[:-2, 1:-1] & both[2:, 1:-1] & both[1:-1, :-2] & both[1:-1, 2:] & both[1:-1, 1:-1]
    sel = interior & edge
    assert np.count_nonzero(sel) > 300
    assert np.abs(got.astype(np.int64) - want)[sel].max() <= 1
    assert abs(int(rec["covered"]) - int(rec0["covered"])) <= 2 * (Ht + Wt)
