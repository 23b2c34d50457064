"""The bilinear stop mask on the device (lf_set_mask_filter): per-ray known answers through lf_generate_lens_rays
against float64 closed forms (a plate behind a stop, the double Gauss), frames of every kernel family against the
nearest lookup of the same function tabulated 64 times finer, and the invariants of the culled march (the support
texture, the grown occupancy, the audit) with the setting's lifecycle.  The CPU oracles do not follow filtered frames:
these tests pin them instead (DESIGN.md sections 4 and 5)."""
import math

import numpy as np
import pytest

from goldenlib import load_texels
from test_gpu_coatings import SUN_NS, _plate, _plate_frame

pytestmark = pytest.mark.gpu
KEY = 0x1e45f1a4e


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="module")
def lf(pkg):
    ctx = pkg.LensFlare(0)
    ctx.set_frame(64, 64)
    ctx.set_aperture(pkg.APERTURE_STARBURST, np.ones((4, 4), np.float32))
    yield ctx
    ctx.close()


def _bil64_texel(t, fu, fv):
    """float64 bilinear interpolation of max(t, 0) at TEXEL coordinates (fu, fv): centres at i + 0.5, indices clamped"""
    h, w = t.shape
    t = np.maximum(t.astype(np.float64), 0.0)
    gx, gy = fu - 0.5, fv - 0.5
    i0, j0 = math.floor(gx), math.floor(gy)
    fx, fy = gx - i0, gy - j0
    xa, xb = min(max(i0, 0), w - 1), min(max(i0 + 1, 0), w - 1)
    ya, yb = min(max(j0, 0), h - 1), min(max(j0 + 1, 0), h - 1)
    a0 = t[ya, xa] + fx * (t[ya, xb] - t[ya, xa])
    a1 = t[yb, xa] + fx * (t[yb, xb] - t[yb, xa])
    return a0 + fy * (a1 - a0)


# ---- per ray: a plate behind an open stop ----------------------------------------------------------------------------
PLATE_N, PLATE_H = 1.67, 500.0


def _plate_stop_hit(u):
    """where the primary path from the sensor's centre through pupil point h u (20 mm away, in air) meets the stop: 5 mm
    of glass and 2 mm of air further on (float64; u as the float32 the device gets)"""
    hu = float(np.float32(PLATE_H) * np.float32(u))
    tan_t = hu / 20.0
    sin_t = tan_t / math.sqrt(1.0 + tan_t * tan_t)
    sin_g = sin_t / PLATE_N
    return hu + 5.0 * sin_g / math.sqrt(1.0 - sin_g * sin_g) + 2.0 * tan_t


def _plate_u_for(f, n):
    """the pupil coordinate whose ray lands on texel coordinate f of an axis of n texels (bisection on the closed form)"""
    want = (2.0 * f / n - 1.0) * PLATE_H
    lo, hi = -0.9, 0.9
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if _plate_stop_hit(mid) < want:
            lo = mid
        else:
            hi = mid
    return float(np.float32(0.5 * (lo + hi)))


def _plate_rays(pkg, lf, mask, filt, uv):
    lf.set_mask_filter(filt)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    return lf.generate_lens_rays(1, np.zeros((len(uv), 2), np.float32), uv)


@pytest.fixture(scope="module")
def plate(pkg, lf):
    lf.set_frame(64, 64)
    lf.set_lens(_plate(PLATE_N, stop=True))
    yield lf
    lf.set_mask_filter(pkg.MASK_NEAREST)


def test_plate_rays_against_float64_bilinear(pkg, plate):
    lf = plate
    rng = np.random.default_rng(11)
    M = rng.uniform(0.25, 1.0, (8, 8)).astype(np.float32)
    us = np.concatenate([np.linspace(-0.8, 0.8, 41), rng.uniform(-0.8, 0.8, 40)]).astype(np.float32)
    uv = np.concatenate([np.stack([us, np.zeros_like(us)], 1), np.stack([np.zeros_like(us), us], 1)])
    ones = _plate_rays(pkg, lf, np.ones((8, 8), np.float32), pkg.MASK_NEAREST, uv)
    assert np.all(ones[:, 7] == 1.0)
    bil = _plate_rays(pkg, lf, M, pkg.MASK_BILINEAR, uv)
    near = _plate_rays(pkg, lf, M, pkg.MASK_NEAREST, uv)
    assert lf.mask_filter() == pkg.MASK_NEAREST
    assert np.all(bil[:, 7] == 1.0) and np.all(near[:, 7] == 1.0)
    # (geometry does not depend on the filter)
    assert np.array_equal(bil[:, :6], near[:, :6]) and np.array_equal(bil[:, :6], ones[:, :6])
    worst, n_near = 0.0, 0
    for k, (u, v) in enumerate(uv):
        fu = (_plate_stop_hit(u) / PLATE_H + 1.0) * 4.0
        fv = (_plate_stop_hit(v) / PLATE_H + 1.0) * 4.0
        want = _bil64_texel(M, fu, fv)
        got = float(bil[k, 6]) / float(ones[k, 6])
        worst = max(worst, abs(got / want - 1.0))
        assert got == pytest.approx(want, rel=2e-5), (u, v, fu, fv)
        # the default filter: the texel hit (away from a texel's edge, where float32 and float64 may land apart; the
        # axis the ray does not move along sits on an edge exactly, at 4.0)
        f = fu if v == 0.0 else fv
        if abs(f - round(f)) > 1e-3:
            n_near += 1
            tex = M[4, int(f)] if v == 0.0 else M[int(f), 4]
            assert float(near[k, 6]) / float(ones[k, 6]) == pytest.approx(float(tex), rel=2e-6), (u, v)
    print("worst relative deviation from the float64 bilinear:", worst)
    assert n_near > 100
    assert not np.allclose(bil[:, 6], near[:, 6], rtol=1e-3)


def test_plate_hard_edge_liveness(pkg, plate):
    lf = plate
    E = np.zeros((8, 8), np.float32)
    E[:, 4:] = 1.0
    inside = np.array([3.6, 3.7, 3.75, 3.8, 3.9, 3.95])          # fu in [3.5, 4): texel 3 (closed), beside texel 4 (open)
    outside = np.array([0.5, 2.0, 3.0, 3.25, 3.4, 3.45])         # both texels of the footprint closed
    for axis in (0, 1):
        mask = E if axis == 0 else E.T.copy()
        uv = np.zeros((12, 2), np.float32)
        uv[:, axis] = [_plate_u_for(f, 8) for f in np.concatenate([inside, outside])]
        ones = _plate_rays(pkg, lf, np.ones((8, 8), np.float32), pkg.MASK_NEAREST, uv)
        bil = _plate_rays(pkg, lf, mask, pkg.MASK_BILINEAR, uv)
        near = _plate_rays(pkg, lf, mask, pkg.MASK_NEAREST, uv)
        assert np.all(ones[:, 7] == 1.0)
        assert np.all(bil[:6, 7] == 1.0) and np.all(bil[6:, 7] == 0.0) and np.all(bil[6:, 6] == 0.0)
        assert np.all(near[:, 7] == 0.0) and np.all(near[:, 6] == 0.0)
        for k in range(6):
            fx = (_plate_stop_hit(uv[k, axis]) / PLATE_H + 1.0) * 4.0 - 3.5
            assert 0.05 < fx < 0.5
            assert float(bil[k, 6]) / float(ones[k, 6]) == pytest.approx(fx, rel=2e-5), (axis, k)


# ---- per ray: the double Gauss -------------------------------------------------------------------------------------

def test_double_gauss_rays_against_float64_bilinear(pkg, lf):
    lf.set_frame(64, 64)
    lf.set_lens(pkg.load_lens_file("dgauss11.lens"))
    n = 16
    g = (np.arange(24) + 0.5) / 12.0 - 1.0
    uv = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2).astype(np.float32)
    xy = np.zeros_like(uv)
    xy[len(uv) // 2:] = (3.0, -2.0)            # half of them from a point off the axis
    ramp = ((np.arange(n) + 0.5) / n).astype(np.float32)
    rng = np.random.default_rng(12)
    M = rng.uniform(0.25, 1.0, (n, n)).astype(np.float32)
    try:
        lf.set_mask_filter(pkg.MASK_BILINEAR)
        res = {}
        for name, mask in (("ones", np.ones((n, n), np.float32)), ("x", np.tile(ramp, (n, 1))),
                           ("y", np.tile(ramp[:, None], (1, n))), ("M", M)):
            lf.set_aperture(pkg.APERTURE_STARBURST, mask)
            assert lf.mask_filter() == pkg.MASK_BILINEAR          # lf_set_aperture keeps the setting
            res[name] = lf.generate_lens_rays(1, xy, uv).astype(np.float64)
    finally:
        lf.set_mask_filter(pkg.MASK_NEAREST)
    alive = res["ones"][:, 7] == 1.0
    for k in ("x", "y", "M"):
        assert np.array_equal(res[k][:, 7] == 1.0, alive)
    # a ramp is exact in the interior: the two ramps give each ray's stop hit in texel coordinates
    fu = n * res["x"][alive, 6] / res["ones"][alive, 6]
    fv = n * res["y"][alive, 6] / res["ones"][alive, 6]
    got = res["M"][alive, 6] / res["ones"][alive, 6]
    use = (fu >= 1.0) & (fu <= n - 1.0) & (fv >= 1.0) & (fv <= n - 1.0)
    assert use.sum() > 100
    worst = 0.0
    for a, b, c in zip(fu[use], fv[use], got[use]):
        want = _bil64_texel(M, a, b)
        worst = max(worst, abs(c / want - 1.0))
        assert c == pytest.approx(want, rel=2e-5), (a, b)
    print("worst relative deviation from the float64 bilinear:", worst, "rays", int(use.sum()))


def test_double_gauss_alive_set_contains_the_nearest_one(pkg, lf, pent):
    """the pentagon mask, ray by ray and without a weight in it: whatever survives the stop under nearest survives it
    under bilinear, the ray is the same ray, and the bilinear set is larger by the half texel around the open region"""
    lf.set_frame(64, 64)
    lf.set_lens(pkg.load_lens_file("dgauss11.lens"))
    g = (np.arange(128) + 0.5) / 64.0 - 1.0
    uv = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2).astype(np.float32)
    xy = np.zeros_like(uv)
    xy[len(uv) // 2:] = (3.0, -2.0)
    try:
        near = _rays_under(pkg, lf, pent, pkg.MASK_NEAREST, xy, uv)
        bil = _rays_under(pkg, lf, pent, pkg.MASK_BILINEAR, xy, uv)
    finally:
        lf.set_mask_filter(pkg.MASK_NEAREST)
    a_near, a_bil = near[:, 7] == 1.0, bil[:, 7] == 1.0
    print("alive under nearest:", int(a_near.sum()), "under bilinear:", int(a_bil.sum()))
    assert a_near.sum() > 1000
    assert not np.any(a_near & ~a_bil)
    assert (a_bil & ~a_near).sum() > 0
    assert np.array_equal(near[a_near, :6], bil[a_near, :6])


def _rays_under(pkg, lf, mask, filt, xy, uv):
    lf.set_mask_filter(filt)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    return lf.generate_lens_rays(1, xy, uv)


# ---- frames: every kernel family ----------------------------------------------------------------------------------
STEP = np.array([[0.0, 0.0, 1.0, 1.0],
                 [0.0, 1.0, 1.0, 0.5],
                 [1.0, 1.0, 0.5, 0.0],
                 [1.0, 0.25, 0.0, 0.0]], np.float32)


def _fine_table(M, k=64):
    """M's bilinear function at the centres of a grid k times finer (k even: no fine texel straddles a half-texel line)"""
    h, w = M.shape
    out = np.zeros((h * k, w * k), np.float64)
    for j in range(h * k):
        for i in range(w * k):
            out[j, i] = _bil64_texel(M, (i + 0.5) / k, (j + 0.5) / k)
    return out.astype(np.float32)


@pytest.fixture(scope="module")
def fine_step():
    return _fine_table(STEP)


@pytest.mark.parametrize("cull,bits", [(0, 6), (2, 6), (0, 0), (2, 0)])
def test_frames_against_the_tabulated_function(pkg, lf, fine_step, cull, bits):
    """pair (1, 2) of a plate behind a stop and the primary path, each crossing the stop once: the bilinear frame of a
    4 x 4 mask against the nearest frame of its bilinear function tabulated on 256 x 256.  A ray lies within half a fine
    texel of that texel's centre on either axis, and the function's slope is at most dM (the largest step between
    neighbouring texels) per coarse texel and axis: |A - B| <= O dM / 64 per pixel, O the frame of the open stop, plus the
    truncation of the fixed-point sums."""
    dM = max(np.abs(np.diff(STEP, axis=0)).max(), np.abs(np.diff(STEP, axis=1)).max())
    lf.test_knob("cull_force", 1)
    try:
        for pairs, primary in (([[1, 2]], False), ([[-1, -1]], False)):
            _plate_frame(pkg, lf, pairs, primary)
            lf.set_pupil_subcells(bits)
            lf.set_march_culling(cull)
            frames = {}
            for name, mask, filt in (("A", STEP, pkg.MASK_BILINEAR), ("B", fine_step, pkg.MASK_NEAREST),
                                     ("O", np.ones((4, 4), np.float32), pkg.MASK_NEAREST), ("N", STEP, pkg.MASK_NEAREST)):
                lf.set_mask_filter(filt)
                lf.set_aperture(pkg.APERTURE_STARBURST, mask)
                lf.trace_ghosts(64, 11)
                frames[name] = lf.read_buffer(pkg.GHOST_BUFFER).copy()
                assert lf.cull_info()["culled"] == (cull != 0), (name, lf.cull_reason())
            fix = lf.march_fix_bits()
            A, B, O, N = (frames[k] for k in "ABON")
            bound = O * (float(dM) / 64.0) * (1.0 + 1e-3) + 2.0 * 64 * 2.0 ** -fix
            err = np.abs(A - B)
            print(pairs, "max |A - B| / bound:", float((err / bound).max()), "max |A - N| / max bound:",
                  float(np.abs(A - N).max() / bound.max()))
            assert (O > 0).sum() > 100
            assert np.all(err <= bound), (pairs, float((err / bound).max()))
            # the comparison can tell the filters apart
            assert np.abs(A - N).max() > 4.0 * bound.max()
    finally:
        lf.test_knob("cull_force", 0)
        lf.set_march_culling(1)
        lf.set_pupil_subcells(6)
        lf.set_mask_filter(pkg.MASK_NEAREST)


# ---- the c3 band: the culled march's invariants and the lifecycle ---------------------------------------------------

def _band(pkg, lf, mask, filt, spp=16, cull=2, y0=512, y1=576, lens=None):
    W, H = 1920, 1080
    lens = lens or pkg.load_lens_file("dgauss11.lens")
    lf.set_frame(W, H)
    lf.set_mask_filter(filt)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    efl = pkg.paraxial_efl(lens)
    sw = lens["sensor_width_mm"]
    lf.set_sun([(SUN_NS[0] - 0.5) * sw / efl, (SUN_NS[1] - 0.5) * sw * H / W / efl, -1.0], [1.0, 0.9, 0.5], 0.05)
    lf.set_ghost_pairs(None, True)
    lf.set_band(y0, y1)
    lf.set_march_culling(cull)
    lf.reset_counters()
    lf.trace_ghosts(spp, KEY)
    assert lf.mask_filter() == filt           # lf_set_aperture, lf_set_lens and lf_set_frame keep the setting
    return dict(ghost=lf.read_buffer(pkg.GHOST_BUFFER).copy(), counters=lf.counters(), executed=lf.executed_events(),
                stats=lf.march_stats(), fix=lf.march_fix_bits(), table=lf.cull_table(), audit=lf.cull_audit(),
                culled=lf.cull_info()["culled"], reason=lf.cull_reason())


@pytest.fixture(scope="module")
def pent():
    return load_texels("pentbig500_14.png")


def _restore(pkg, lf):
    lf.test_knob("cull_force", 0)
    lf.test_knob("cull_weights_first", 0)
    lf.set_pupil_subcells(6)
    lf.set_march_culling(1)
    lf.set_mask_filter(pkg.MASK_NEAREST)
    lf.set_frame(64, 64)                  # (the whole frame is the band again)


def test_kernels_agree_bit_for_bit_under_the_filter(pkg, lf, pent):
    lf.test_knob("cull_force", 1)
    try:
        F = pkg.MASK_BILINEAR
        full = _band(pkg, lf, pent, F, cull=0)
        culled = _band(pkg, lf, pent, F, cull=2)
        assert culled["culled"] and not full["culled"]
        assert culled["reason"] == "applied"
        assert culled["audit"]["rays"] > 0 and culled["audit"]["lit"] == 0 and culled["audit"]["launches_refuted"] == 0
        assert np.array_equal(full["ghost"], culled["ghost"])
        assert full["counters"]["rays_hit_light"] == culled["counters"]["rays_hit_light"]
        assert full["ghost"].sum() > 0
        lf.test_knob("cull_weights_first", 1)
        try:
            wf = _band(pkg, lf, pent, F, cull=2)
        finally:
            lf.test_knob("cull_weights_first", 0)
        assert wf["culled"] and np.array_equal(wf["ghost"], culled["ghost"])
        # against the default filter: the lit set only grows, the stop clips no more rays than before
        near_full = _band(pkg, lf, pent, pkg.MASK_NEAREST, cull=0)
        near = _band(pkg, lf, pent, pkg.MASK_NEAREST, cull=2)
        assert np.array_equal(near_full["ghost"], near["ghost"])
        assert full["counters"]["rays_clipped_stop"] <= near_full["counters"]["rays_clipped_stop"]
        assert full["counters"]["rays_hit_light"] >= near_full["counters"]["rays_hit_light"]
        # the lit RAYS contain the nearest filter's (test_double_gauss_alive_set_contains_the_nearest_one holds that per
        # ray); in the pixels a ray alive under nearest keeps at least 1/4 of its weight per crossing of the stop (its own
        # texel enters with (1 - fx)(1 - fy) >= 1/4, the others with >= 0) and a path of this lens crosses the stop up to
        # three times: 1/64.  A pixel sums at most spp x paths contributions per channel, each truncated to the 2^-fix
        # grid once, so a value lit under nearest can vanish here only below 64 x that
        grid = 16 * 46 * 2.0 ** -culled["fix"]            # 16 spp x (45 pairs + the primary path)
        gone = (near["ghost"] > 0) & ~(culled["ghost"] > 0)
        print("lit under nearest only:", int(gone.sum()), "of", int((near["ghost"] > 0).sum()), "largest",
              float(near["ghost"][gone].max()) if gone.any() else 0.0, "grid bound", 64 * grid)
        assert np.all(culled["ghost"] >= near["ghost"] * ((1 - 1e-5) / 64.0) - grid)
        assert not gone.any() or near["ghost"][gone].max() <= 64 * grid * (1 + 1e-5)
        assert not np.array_equal(near["ghost"], culled["ghost"])
        # the independent-pixel item kernel against the path tree, one sampling specification
        lf.set_pupil_subcells(0)
        tree = _band(pkg, lf, pent, F, cull=0)
        items = _band(pkg, lf, pent, F, cull=2)
        assert items["culled"] and items["audit"]["lit"] == 0
        assert np.array_equal(tree["ghost"], items["ghost"])
        assert tree["ghost"].sum() > 0
    finally:
        _restore(pkg, lf)


def test_an_open_mask_does_not_see_the_filter(pkg, lf):
    # (a fully open stop starts more of the table than the culled kernel is worth -- "table_too_full" -- so the knob
    # holds the launch to it: the table is part of what is compared)
    lf.test_knob("cull_force", 1)
    try:
        ones = np.ones((500, 500), np.float32)
        a = _band(pkg, lf, ones, pkg.MASK_NEAREST)
        b = _band(pkg, lf, ones, pkg.MASK_BILINEAR)
        assert a["culled"] and b["culled"], (a["reason"], b["reason"])
        assert a["reason"] == b["reason"] == "applied"
        assert np.array_equal(a["ghost"], b["ghost"]) and a["ghost"].sum() > 0
        for k in ("counters", "executed", "stats", "audit"):
            assert a[k] == b[k], k
        assert np.array_equal(a["table"], b["table"])
    finally:
        _restore(pkg, lf)


def test_lifecycle(pkg, lf, pent):
    # (at 16 samples the table's cells are coarse and it starts more than the culled kernel is worth: the knob holds the
    # launches to it, the table's lifetime is part of what is checked)
    lf.test_knob("cull_force", 1)
    try:
        never = _band(pkg, lf, pent, pkg.MASK_NEAREST)
        assert never["culled"], never["reason"]
        # on, then off again: the frame of a context that never had the filter
        lf.set_mask_filter(pkg.MASK_BILINEAR)
        lf.trace_ghosts(16, KEY)
        filtered = lf.read_buffer(pkg.GHOST_BUFFER).copy()
        assert not np.array_equal(filtered, never["ghost"])
        lf.set_mask_filter(pkg.MASK_NEAREST)
        assert lf.mask_filter() == pkg.MASK_NEAREST
        lf.trace_ghosts(16, KEY)
        assert np.array_equal(lf.read_buffer(pkg.GHOST_BUFFER), never["ghost"])
        # set before the mask and the lens = switched afterwards
        assert np.array_equal(_band(pkg, lf, pent, pkg.MASK_BILINEAR)["ghost"], filtered)
        with pytest.raises(pkg.LensFlareError, match="LF_ERR_INVALID"):
            lf.set_mask_filter(2)
        assert lf.mask_filter() == pkg.MASK_BILINEAR
        # culling mode 1 keeps its table between launches: a switch rebuilds it
        m2_near = _band(pkg, lf, pent, pkg.MASK_NEAREST, cull=2)["ghost"]
        lf.set_march_culling(1)
        lf.trace_ghosts(16, KEY)
        assert lf.cull_info()["culled"], lf.cull_reason()
        assert np.array_equal(lf.read_buffer(pkg.GHOST_BUFFER), m2_near)
        lf.set_mask_filter(pkg.MASK_BILINEAR)
        lf.trace_ghosts(16, KEY)
        assert lf.cull_info()["culled"], lf.cull_reason()
        assert np.array_equal(lf.read_buffer(pkg.GHOST_BUFFER), filtered)
        lf.set_mask_filter(pkg.MASK_NEAREST)
        lf.trace_ghosts(16, KEY)
        assert np.array_equal(lf.read_buffer(pkg.GHOST_BUFFER), m2_near)
        # the lens camera's calibration follows the filter.  A soft edge across the open stop, the open side reaching the
        # housing: the stop's chord grows towards the axis, so the bilinear ramp gains more light on the inner side of
        # each step than it loses on the outer one (about 2 % of the nearest filter's)
        lf.set_frame(64, 64)
        soft = np.tile(np.array([1.0, 0.5, 0.0, 0.0], np.float32), (4, 1))
        lf.set_aperture(pkg.APERTURE_STARBURST, soft)
        lf.set_lens_camera(1, 0.001, 0.0)
        e_near = lf.lens_camera()["exposure"]
        lf.set_mask_filter(pkg.MASK_BILINEAR)
        e_bil = lf.lens_camera()["exposure"]
        assert abs(e_bil / e_near - 1.0) > 1e-3
        lf.set_mask_filter(pkg.MASK_NEAREST)
        assert lf.lens_camera()["exposure"] == e_near
        lf.set_lens_camera(0, 0.001, 0.0)
    finally:
        _restore(pkg, lf)
