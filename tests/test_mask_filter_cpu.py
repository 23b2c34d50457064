"""The stop-mask lookup, host side (no device): lf_mask_lookup -- the float32 contract of LF_MASK_BILINEAR and of the
default nearest texel (lf_march_events.h: lf_mask_bilinear / stop_event) evaluated on the host -- against its closed
forms, its borders, its liveness rule, its refusals and an independent float64 bilinear interpolation written here."""
import ctypes as C
import math

import numpy as np
import pytest


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def _u_of(f, n):
    """the stop-plane coordinate that lands on texel coordinate f of an axis of n texels"""
    return 2.0 * f / n - 1.0


def _fu32(u, n):
    """the march's float32 texel coordinate: fmaf(u, 1, 1) * (0.5f * n)"""
    return np.float32(np.float32(u) + np.float32(1.0)) * np.float32(0.5 * n)


def bilinear64(t, u, v):
    """float64 bilinear interpolation of max(t, 0), texel centres at i + 0.5, indices clamped; (value, any of four open)"""
    h, w = t.shape
    t = np.maximum(t.astype(np.float64), 0.0)
    gx = (float(np.float32(u)) + 1.0) * 0.5 * w - 0.5
    gy = (float(np.float32(v)) + 1.0) * 0.5 * h - 0.5
    i0, j0 = math.floor(gx), math.floor(gy)
    fx, fy = gx - i0, gy - j0
    xa, xb = min(max(i0, 0), w - 1), min(max(i0 + 1, 0), w - 1)
    ya, yb = min(max(j0, 0), h - 1), min(max(j0 + 1, 0), h - 1)
    a0 = t[ya, xa] + fx * (t[ya, xb] - t[ya, xa])
    a1 = t[yb, xa] + fx * (t[yb, xb] - t[yb, xa])
    return a0 + fy * (a1 - a0), max(t[ya, xa], t[ya, xb], t[yb, xa], t[yb, xb]) > 0.0


def test_texel_centres_return_the_texel():
    pkg = _pkg()
    t = np.random.default_rng(1).random((4, 8)).astype(np.float32)
    for j in range(4):
        for i in range(8):
            value, alive = pkg.mask_lookup(t, _u_of(i + 0.5, 8), _u_of(j + 0.5, 4), pkg.MASK_BILINEAR)
            assert value == float(t[j, i]) and alive == 1


def test_a_ramp_is_reproduced_in_the_interior():
    pkg = _pkg()
    w, h = 8, 4
    t = np.tile(((np.arange(w) + 0.5) / w).astype(np.float32), (h, 1))
    bound = 2.0 * (3 + 2 * w) * 2.0 ** -24
    for fu in np.linspace(0.5, w - 0.5, 57):
        for fv in (0.3, 1.0, 2.71, 3.9):
            value, alive = pkg.mask_lookup(t, _u_of(fu, w), _u_of(fv, h))
            assert alive == 1
            assert abs(value - float(_fu32(_u_of(fu, w), w)) / w) <= bound, (fu, fv)


def test_borders_clamp():
    pkg = _pkg()
    t = np.random.default_rng(2).random((4, 8)).astype(np.float32) + 0.1
    vc = _u_of(1.5, 4)     # the centre of row 1
    for u, i in ((-1.0, 0), (_u_of(0.25, 8), 0), (-1.5, 0), (-1e30, 0), (1.0, 7), (_u_of(7.75, 8), 7), (2.0, 7), (1e30, 7)):
        assert pkg.mask_lookup(t, u, vc) == (float(t[1, i]), 1), u
    uc = _u_of(2.5, 8)
    for v, j in ((-1.0, 0), (-3.0, 0), (1.0, 3), (_u_of(3.6, 4), 3), (7.0, 3)):
        assert pkg.mask_lookup(t, uc, v) == (float(t[j, 2]), 1), v
    # a single texel is the whole plane
    one = np.array([[0.625]], np.float32)
    for u, v in ((0.0, 0.0), (-0.9, 0.7), (5.0, -5.0)):
        assert pkg.mask_lookup(one, u, v) == (0.625, 1)


def test_negative_texels_count_as_zero():
    pkg = _pkg()
    t = np.array([[-1.0, 0.5, -2.0, -3.0]], np.float32)
    # half way between texel 0 (-1 -> 0) and texel 1 (0.5)
    assert pkg.mask_lookup(t, _u_of(1.0, 4), 0.0) == (0.25, 1)
    # between the two negative texels: closed, and the value is 0, not negative
    assert pkg.mask_lookup(t, _u_of(3.0, 4), 0.0) == (0.0, 0)
    assert pkg.mask_lookup(t, _u_of(3.5, 4), 0.0, pkg.MASK_NEAREST) == (-3.0, 0)


def test_open_is_any_of_the_four_texels():
    pkg = _pkg()
    t = np.array([[0.0, 0.0, 1.0, 1.0]], np.float32)
    # fu = 1.5: gx = 1 exactly, fx == 0 with texel 2 open beside it: weight 0, alive
    assert pkg.mask_lookup(t, _u_of(1.5, 4), 0.0) == (0.0, 1)
    # inside the half texel next to the edge: alive, weight fx
    assert pkg.mask_lookup(t, _u_of(1.75, 4), 0.0) == (0.25, 1)
    # further out both texels are closed
    assert pkg.mask_lookup(t, _u_of(1.4375, 4), 0.0) == (0.0, 0)
    # nearest: the texel hit decides
    assert pkg.mask_lookup(t, _u_of(1.75, 4), 0.0, pkg.MASK_NEAREST) == (0.0, 0)
    assert pkg.mask_lookup(t, _u_of(2.0, 4), 0.0, pkg.MASK_NEAREST) == (1.0, 1)
    # ... and in y
    assert pkg.mask_lookup(t.T.copy(), 0.0, _u_of(1.5, 4)) == (0.0, 1)
    assert pkg.mask_lookup(t.T.copy(), 0.0, _u_of(1.25, 4)) == (0.0, 0)


def test_nearest_reproduces_the_texel_hit():
    pkg = _pkg()
    rng = np.random.default_rng(3)
    t = (rng.random((5, 7)) - 0.3).astype(np.float32)
    for u, v in rng.uniform(-1.2, 1.2, (300, 2)).astype(np.float32):
        ix = min(max(int(_fu32(u, 7)), 0), 6)
        iy = min(max(int(_fu32(v, 5)), 0), 4)
        assert pkg.mask_lookup(t, u, v, pkg.MASK_NEAREST) == (float(t[iy, ix]), int(t[iy, ix] > 0)), (u, v)


def test_bilinear_contains_nearest():
    pkg = _pkg()
    rng = np.random.default_rng(4)
    t = (rng.random((5, 7)) < 0.4).astype(np.float32)
    for u, v in rng.uniform(-1.1, 1.1, (300, 2)).astype(np.float32):
        if pkg.mask_lookup(t, u, v, pkg.MASK_NEAREST)[1]:
            assert pkg.mask_lookup(t, u, v, pkg.MASK_BILINEAR)[1] == 1


def test_against_float64_bilinear_at_random_points():
    pkg = _pkg()
    rng = np.random.default_rng(5)
    w, h = 7, 5
    t = rng.random((h, w)).astype(np.float32)
    # three fused lerps, plus the two roundings in forming fu times the slope (texels in [0, 1]: at most 1 per texel);
    # twice that is allowed
    bound = 2.0 * (3 + 2 * w) * 2.0 ** -24
    worst = 0.0
    for u, v in rng.uniform(-1.0, 1.0, (1000, 2)).astype(np.float32):
        value, alive = pkg.mask_lookup(t, u, v)
        want, want_alive = bilinear64(t, u, v)
        worst = max(worst, abs(value - want))
        assert alive == int(want_alive)
    print("worst |float32 - float64| =", worst, "bound", bound)
    assert worst <= bound


def test_bad_arguments_are_refused():
    pkg = _pkg()
    lib = pkg.load_library()
    t = np.ones((2, 2), np.float32)
    p = t.ctypes.data_as(C.POINTER(C.c_float))
    value, alive = C.c_float(), C.c_int()

    def call(tex, w, h, filt, u, v):
        return lib.lf_mask_lookup(tex, w, h, filt, C.c_float(u), C.c_float(v), C.byref(value), C.byref(alive))

    assert call(p, 2, 2, 1, 0.0, 0.0) == 0
    assert lib.lf_mask_lookup(p, 2, 2, 1, C.c_float(0.0), C.c_float(0.0), None, None) == 0   # either output may be NULL
    for args in ((None, 2, 2, 1, 0.0, 0.0), (p, 0, 2, 1, 0.0, 0.0), (p, 2, -1, 1, 0.0, 0.0), (p, 5000, 2, 1, 0.0, 0.0),
                 (p, 2, 2, 2, 0.0, 0.0), (p, 2, 2, -1, 0.0, 0.0), (p, 2, 2, 1, float("nan"), 0.0),
                 (p, 2, 2, 1, 0.0, float("inf"))):
        assert call(*args) == 1, args
    with pytest.raises(pkg.LensFlareError, match="LF_ERR_INVALID"):
        pkg.mask_lookup(t, 0.0, 0.0, 7)
