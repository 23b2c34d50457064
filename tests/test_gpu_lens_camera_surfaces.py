"""The scene imaged through aspheric and anamorphic lenses (lf_set_lens_camera_surfaces(LF_LENSCAM_SURFACES_ALL); k_scene_lens<..,
SURF>, primary_path_general) and the call that hands out the lens camera's samples (lf_lens_camera_samples):

  1. the samples call against the float32 oracle that exists (spheres), bit for bit;
  2. a recorded lens's frame = the composition of the device's OWN rays (lf_generate_lens_rays at lf_lens_camera_samples), to
     1e-9: every FILT x STACK variant, sampled lights, both modes, an odd frame;
  3. the frame against the float64 Python tracers, the bar taken from the kernels that exist (Q, below);
  4. a known answer: the anamorphic squeeze moves a distant emitter's image where the tracer's chief ray says;
  5. the calibrated exposure against the tracer, and the flat field under lf_set_lens_camera_aim;
  6. nothing else moves: a lens of spheres under ALL, records set and cleared, the per-lane kernel's refusal, the row deal,
     setter and getter.

Every test here needs lf_set_lens_camera_surfaces: none passes on a library without it."""
import math

import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo
from test_geo_rays_vs_f64 import W_TOL
from test_gpu_lens_camera import KEY, LIGHTS, SPHERES, TRIS, compose, sample_order, setup_scene_frame, unit_lights
from lens_camera_surfaces_lib import (ALLOWANCE_CAP, C2W, H, NS, ODD, ONES, POS, W, WPM, films_of, lens_of, trace, tracer_frame,
                                      tracer_samples)

import biconic_ref as br

pytestmark = pytest.mark.gpu
LF_ERR_INVALID, LF_ERR_UNSUPPORTED = 1, 6
TOL = 1e-9                                 # the bar of test_lens_frame_equals_the_float32_oracle


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture()
def lf(pkg):
    ctx = pkg.LensFlare(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def pentagon():
    return load_texels("pentbig500_14.png")


def device_rays(lf, lam, n_pix):
    """(n_pix, ns, 4) starts and (n_pix, ns, 8) exit rays of the lens camera's samples, both the device's own"""
    s = lf.lens_camera_samples(np.arange(n_pix))
    rays = lf.generate_lens_rays(lam, s[..., 0:2], s[..., 2:4]).reshape(s.shape[0], s.shape[1], 8)
    return s, rays


def own_frame(lf, lens, mode, w, h, ns, info):
    """the frame composed from the device's own rays, and how many of them left the lens"""
    want, left = np.zeros((w * h, 3)), 0
    for lam in ((1,) if mode == 1 else (0, 1, 2)):
        _, rays = device_rays(lf, lam, w * h)
        with np.errstate(invalid="ignore"):
            f, _, alive = compose(lens, None, w, h, ns, C2W, POS, WPM, info["entrance_pupil_z_mm"], info["exposure"], rays, 6,
                                  SPHERES, TRIS, LIGHTS)
        left += int(alive.sum())
        if mode == 1:
            want = f
        else:
            want[:, lam] = f[:, lam]       # 3 wavelengths: the identity weights
    return want, left


# ---- 1. the samples call against the oracle that exists -------------------------------------------------------------------
def test_samples_are_the_float32_oracles(pkg, lf, pentagon):
    """dgauss11.lens, the default setting: lf_generate_lens_rays at lf_lens_camera_samples = lfo.geo_lens_samples, the oracle
    that follows the lens camera sample by sample -- fate and weight of every sample, exit point and direction of every sample
    that leaves, bit for bit (the first six values of a blocked ray are whatever the march left: oracle/lf_geo_oracle.c says so
    itself), three wavelengths.  The starts are plausible on their own: inside their pixel, inside the pupil square."""
    lens = lens_of("plain")
    setup_scene_frame(pkg, lf, lens, pentagon, W, H, NS, C2W, POS)
    assert lf.lens_camera_surfaces() == pkg.LENSCAM_SURFACES_SPHERICAL
    s = lf.lens_camera_samples(np.arange(W * H))
    assert s.shape == (W * H, NS, 4) and s.dtype == np.float32
    pitch = 36.0 / W
    y, x = np.divmod(np.arange(W * H), W)
    px = 0.5 * W - s[..., 0] / pitch - x[:, None]
    py = 0.5 * H - s[..., 1] / pitch - y[:, None]
    assert px.min() > -1e-4 and px.max() < 1 + 1e-4 and py.min() > -1e-4 and py.max() < 1 + 1e-4
    assert np.abs(s[..., 2:4]).max() <= 1.0 and s[..., 2].std() > 0.5 and s[..., 3].std() > 0.5
    lfo.geo_follow_device(lf)
    try:
        for lam in (0, 1, 2):
            got = lf.generate_lens_rays(lam, s[..., 0:2], s[..., 2:4]).reshape(W * H, NS, 8)
            want = lfo.geo_lens_samples(lens, W, H, NS, KEY, lam, np.arange(W * H), pentagon)
            assert np.array_equal(got[..., 6:8].view(np.uint32), want[..., 6:8].view(np.uint32)), lam
            alive = want[..., 7] == 1.0
            assert 0.1 < alive.mean() < 0.5
            assert np.array_equal(got[alive].view(np.uint32), want[alive].view(np.uint32)), lam
    finally:
        lfo.geo_follow_device(None)
    # a subset of the pixels, in any order, is the same samples
    pick = np.array([W * H - 1, 0, 7 * W + 5], np.int32)
    assert np.array_equal(lf.lens_camera_samples(pick).view(np.uint32), s[pick].view(np.uint32))
    with pytest.raises(pkg.LensFlareError) as e:
        lf.lens_camera_samples([W * H])
    assert e.value.status == LF_ERR_INVALID


# ---- 2. the frame is the composition of the device's own rays -------------------------------------------------------------
def configure(pkg, lf, name, pentagon, what, w=W, h=H, ns=NS):
    lens = dict(lens_of(name))
    if "films" in what:
        lens["coatings"] = films_of(name)
    if "stacks" in what:
        lens["coating_stacks"] = pkg.load_lens_file("dgauss11_multicoated.lens")["coating_stacks"]
    setup_scene_frame(pkg, lf, lens, pentagon, w, h, ns, C2W, POS)
    lf.set_mask_filter(pkg.MASK_BILINEAR if "bilinear" in what else pkg.MASK_NEAREST)
    lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_ALL)
    lf.set_lens_camera_aim(0.0)
    return lens


OWN_CASES = [("asph", "bare", 1), ("asph", "bare", 2), ("anam", "bare", 1), ("anam", "bare", 2), ("asph", "films", 1),
             ("asph", "stacks", 1), ("asph", "bilinear", 1), ("asph", "stacks-bilinear", 1), ("anam", "bilinear", 2),
             ("asph", "odd", 2), ("anam", "odd", 1)]


@pytest.mark.parametrize("name,what,mode", OWN_CASES, ids=[f"{n}-{w}-mode{m}" for n, w, m in OWN_CASES])
def test_frame_is_the_composition_of_the_devices_own_rays(pkg, lf, pentagon, name, what, mode):
    """Under ALL the frame of a recorded lens = sum_s exposure * weight_s * L(exit ray_s) / (ns + 1) with the exit rays and
    weights lf_generate_lens_rays gives at lf_lens_camera_samples (k_march_path_rays: bit for bit the ray the scene kernel
    queues), exposure and entrance pupil as lens_camera() reports them, the scene oracle's radiance: 1e-9, the bar of
    test_lens_frame_equals_the_float32_oracle, and its counters.  One case per FILT x STACK variant of the SURF = 1 kernels
    (films, stacks, the bilinear stop, stacks and the bilinear stop), SURF = 2 bare and filtered, both modes, and the odd
    frame (no multiple of the tile, unstratified samples).  Measured on an MI355X: 2.5e-16 - 4.6e-16."""
    w, h, ns = ODD if what == "odd" else (W, H, NS)
    lens = configure(pkg, lf, name, pentagon, what, w, h, ns)
    lf.set_lens_camera(mode, WPM, 0.0)
    lf.reset_scene_counters()
    lf.render_scene_term()
    got = lf.read_buffer(pkg.SCENE_BUFFER).reshape(-1, 3)
    info, cnt = lf.lens_camera(), lf.scene_counters()
    assert info["mode"] == mode and info["exposure"] > 0
    z_ep, _ = pkg.paraxial_entrance_pupil(lens)
    assert info["entrance_pupil_z_mm"] == z_ep                 # (the y meridian's: the convention of DESIGN.md section 4)
    want, left = own_frame(lf, lens, mode, w, h, ns, info)
    assert cnt["lens_samples"] == w * h * ns * (3 if mode == 2 else 1) and cnt["lens_left"] == left
    assert (want.max(axis=-1) > 0.02).mean() > 0.5             # not a dark frame
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-12)
    print(f"{name} {what} mode {mode}: {left} of {cnt['lens_samples']} samples leave the lens, largest deviation {err.max():.2e}")
    assert err.max() <= TOL, err.max()


@pytest.mark.parametrize("name", ["asph", "anam"])
def test_frame_with_sampled_lights_is_the_composition_of_the_devices_own_rays(pkg, lf, pentagon, name):
    """SOFT = true: the sun and the area light of test_lens_frame_with_sampled_lights_equals_the_oracle_draw_for_draw.  The
    device's own exit rays go to the float64 scene oracle with the counter the device draws that sample's light samples
    from -- (pixel, sample NUMBER of the loop).  That test's bar and fragility rule (tests/test_gpu_sampled_lights.py)."""
    import sampled_lights_cases as slc
    lens = configure(pkg, lf, name, pentagon, "bare")
    sun = unit_lights(LIGHTS)[0]
    rows = [[0.0] + sun[4:7] + sun[1:4] + [0.0] * 9,
            [3.0, 6.0, 6.0, 5.0, 0.0, 2.5, -5.0, 0.0, -1.0, 0.0, 1.0, 0.0, 0.2, 0.0, 0.3, 1.0]]
    lf.set_scene_lights(rows)
    lf.set_light_samples(3)
    lf.set_lens_camera(1, WPM, 0.0)
    lf.render_scene_term()
    got = lf.read_buffer(pkg.SCENE_BUFFER).reshape(-1, 3)
    info = lf.lens_camera()
    desc = lfo.scene_desc(SPHERES, TRIS, rows, 3, False, None)
    number = np.empty(NS, np.uint32)
    number[sample_order(NS)] = np.arange(1, NS + 1)          # march sample -> sample number
    ctr = np.stack([np.repeat(np.arange(W * H, dtype=np.uint32), NS), np.tile(number, W * H)], -1)
    _, smp = device_rays(lf, 1, W * H)
    alive = (smp[..., 6] > 0).reshape(-1)
    with np.errstate(invalid="ignore"):
        o, d = lfo.lens_exit_to_world(smp[..., 0:3], smp[..., 3:6], C2W, POS, WPM, info["entrance_pupil_z_mm"])
    rays = np.concatenate([o, d, np.full(o.shape[:-1] + (1,), 0.01), np.full(o.shape[:-1] + (1,), 100.0)], -1)
    L = np.zeros((W * H * NS, 3))
    out, frag = lfo.scene_rays(desc, rays.reshape(-1, 8)[alive], ctr[alive], KEY)
    L[alive] = out[:, 5:8]
    fr = np.zeros(W * H * NS, bool)
    fr[alive] = frag
    fragile = fr.reshape(W * H, NS).any(axis=1)
    wgt = smp[..., 6].astype(np.float64).reshape(-1) * info["exposure"]
    want = (L * wgt[:, None]).reshape(W * H, NS, 3).sum(axis=1) / (NS + 1)
    assert (want.max(axis=-1) > 0.02).mean() > 0.5 and fragile.sum() <= slc.PIXEL_CAP * W * H, fragile.sum()
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    err[got == want] = 0.0
    print(f"{name} sampled lights: {int(fragile.sum())} fragile pixels, largest deviation {err[~fragile].max():.3e}")
    assert err[~fragile].max() <= slc.TOL


# ---- 3. the frame against float64 -----------------------------------------------------------------------------------------
_device = {}


def device_frame(pkg, lf, name, filmed, mode):
    """(frame, lens_camera() info, per wavelength the device's starts) under a mask of ones, rendered once per case"""
    key = (name, filmed, mode)
    if key not in _device:
        lens = dict(lens_of(name))
        if filmed:
            lens["coatings"] = films_of(name)
        setup_scene_frame(pkg, lf, lens, ONES, W, H, NS, C2W, POS)
        lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_SPHERICAL if name == "plain" else pkg.LENSCAM_SURFACES_ALL)
        lf.set_lens_camera(mode, WPM, 0.0)
        lf.render_scene_term()
        _device[key] = (lf.read_buffer(pkg.SCENE_BUFFER).reshape(-1, 3), lf.lens_camera(), lf.lens_camera_samples(np.arange(W * H)))
    return _device[key]


def against_tracer(pkg, lf, name, filmed, mode, traced_as=None):
    """(device frame, tracer frame, allowance) of a case; traced_as: the lens the TRACER follows (the neighbour clause)"""
    got, info, starts = device_frame(pkg, lf, name, filmed, mode)
    want, allow = np.zeros_like(got), np.zeros_like(got)
    for lam in ((1,) if mode == 1 else (0, 1, 2)):
        t = trace(traced_as or name, lam, starts, "device")
        f, a = tracer_frame(traced_as or name, t, filmed, (W * H, NS), info["entrance_pupil_z_mm"], info["exposure"])
        if mode == 1:
            want, allow = f, a
        else:
            want[:, lam], allow[:, lam] = f[:, lam], a[:, lam]
    return got, want, allow


def yardstick_q(pkg, lf, filmed, mode):
    """Q: dgauss11.lens under the default setting -- the kernels that exist -- against the same tracer at the device's samples:
    the largest relative deviation of a lit value (want > 1e-3) outside the allowance"""
    got, want, allow = against_tracer(pkg, lf, "plain", filmed, mode)
    assert allow.sum() < ALLOWANCE_CAP * want.sum()
    lit = want > 1e-3
    q = float(np.max(np.maximum(np.abs(got - want) - allow, 0.0)[lit] / want[lit]))
    return q, int(lit.sum())


F64_CASES = [("asph", False, 1), ("asph", True, 1), ("anam", False, 1), ("anam", True, 1), ("anam", False, 2)]


@pytest.mark.parametrize("name,filmed,mode", F64_CASES, ids=[f"{n}-{'filmed' if f else 'bare'}-mode{m}" for n, f, m in F64_CASES])
def test_frame_against_the_float64_tracers(pkg, lf, name, filmed, mode):
    """The reference: asphere_ref / biconic_ref trace_path(lens, lam, -1, -1, ...) at the device's samples, a mask of ones,
    composed by compose.  A sample the tracer finds within 4 D n_ev of an aperture rim or at incidence cosine <= 0.05 is
    fragile: its allowance is its weight times the radiance its ray finds (one the tracer killed: the frame's largest weight
    and radiance), all of them together below 2 % of the frame's summed value.  The bar comes from code that exists: Q, the
    largest relative deviation of a lit value outside the allowance when dgauss11.lens under the default setting meets the
    same tracer the same way, Q <= 2e-3 (the outermost bar of the existing float64 frame test: a bad yardstick fails and
    widens nothing); every value of a recorded frame within 4 Q + allowance.  And the comparison tells the records: the device
    frame misses the tracer's frame of the lens with its records dropped by more than ten times what it misses its own by
    (mode 1; the CPU test confirms the tracer's side).  Measured on an MI355X: Q = 1.13e-4 bare and filmed; the worst
    deviation outside the allowance 0.20 Q (aspheric), 0.46 Q (anamorphic) and 0.55 Q (anamorphic, mode 2); allowance 0.24 %
    and 0.87 % of the frame; own miss 2e-7 - 3e-7 of the sum, records dropped 0.10 and 0.29."""
    q, n_lit = yardstick_q(pkg, lf, filmed, mode)
    print(f"yardstick {'filmed' if filmed else 'bare'} mode {mode}: Q = {q:.3e} over {n_lit} lit values")
    assert 0.0 < q <= 2e-3, q
    got, want, allow = against_tracer(pkg, lf, name, filmed, mode)
    share = allow.sum() / want.sum()
    assert share < ALLOWANCE_CAP, share
    assert (want.max(axis=-1) > 0.02).mean() > 0.5
    dev = np.abs(got - want)
    over = dev - allow
    lit = want > 1e-3
    ratio = float(np.max(np.maximum(over, 0.0)[lit] / want[lit]) / q)
    print(f"{name} {'filmed' if filmed else 'bare'} mode {mode}: allowance {share:.2e} of the frame, worst deviation outside "
          f"it {ratio:.3f} of Q (bar 4), median relative deviation {np.median(dev[lit] / want[lit]):.2e}")
    assert (dev <= 4.0 * q * np.abs(want) + allow).all(), float(np.max((over - 4.0 * q * np.abs(want))))
    if mode == 1:
        _, other, _ = against_tracer(pkg, lf, name, filmed, mode, traced_as=name + "-dropped")
        own_miss, other_miss = float(np.abs(got - want).sum() / want.sum()), float(np.abs(got - other).sum() / want.sum())
        print(f"  summed |device - tracer| / summed tracer: own {own_miss:.2e}, records dropped {other_miss:.2e}")
        assert other_miss > 10.0 * own_miss


# ---- 4. known answer: the squeeze -----------------------------------------------------------------------------------------
def centroid(img):
    lum = img.sum(axis=-1)
    yy, xx = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    return float((lum * (xx + 0.5)).sum() / lum.sum()), float((lum * (yy + 0.5)).sum() / lum.sum())


def test_a_distant_emitter_lands_where_the_chief_ray_says(pkg, lf):
    """The anamorphic lens, a small emissive sphere 50 m away along the world direction into which the float64 tracer sends
    the chief ray (pupil point 0, 0) of the sensor point (6, 4) mm: the centroid of the device's image lies at that sensor
    point.  The tolerance is measured: the float64-composed frame (the tracer at the device's samples of the pixels around
    the point) has a centroid of its own, off the chief ray's prediction by the lens's aberrations and the pixel raster --
    twice that offset, plus 0.1 pixel for the float32 noise of a centroid.  The same sphere through dgauss11.lens: the
    centroids' x : y offset ratios differ by the ratio of lf_get_lens_meridian_scales, within that tolerance propagated.
    Measured on an MI355X: predicted (32.000, 21.333), float64-composed and device centroid both (32.008, 21.380), tolerance
    0.194 px; ratio 0.7575 against 0.7495 under a propagated tolerance of 5.7 %."""
    Wk, Hk, ns, wpm = 96, 64, 16, 0.001
    X0, Y0, dist, radius = 6.0, 4.0, 50.0, 0.6
    lens, plain = lens_of("anam"), lens_of("plain")
    eye, origin = np.eye(3).reshape(-1), [0.0, 0.0, 0.0]
    z_ep, _ = pkg.paraxial_entrance_pupil(lens)
    chief = br.trace_path(lens, 1, -1, -1, [[X0, Y0]], [[0.0, 0.0]], ONES)[0][0]
    assert chief[7] == 1.0
    o = np.array([chief[0], chief[1], chief[2] - z_ep]) * wpm
    d = chief[3:6] / np.linalg.norm(chief[3:6])
    emitter = [tuple(o + dist * d) + (radius, "e", 5.0, 5.0, 5.0)]
    setup_scene_frame(pkg, lf, lens, ONES, Wk, Hk, ns, eye, origin, spheres=emitter, tris=[], lights=[])
    lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_ALL)
    lf.set_lens_camera(1, wpm, 0.0)
    lf.render_scene_term()
    img = lf.read_buffer(pkg.SCENE_BUFFER)
    info = lf.lens_camera()
    sx, sy = lf.lens_meridian_scales()
    pitch = 36.0 / Wk
    pred = (0.5 * Wk - X0 / pitch, 0.5 * Hk - Y0 / pitch)
    got = centroid(img)
    lit = img.sum(axis=-1) > 0.04 * img.sum(axis=-1).max()
    assert 4 <= lit.sum() <= 60, lit.sum()                      # a few pixels
    # the float64-composed frame over the pixels around the prediction (every lit pixel of the device's frame is inside)
    x0, y0 = int(pred[0]) - 8, int(pred[1]) - 8
    ys, xs = np.mgrid[y0:y0 + 17, x0:x0 + 17]
    assert lit[y0:y0 + 17, x0:x0 + 17].sum() == lit.sum()
    pix = (ys * Wk + xs).reshape(-1)
    s = lf.lens_camera_samples(pix)
    t = br.trace_path(lens, 1, -1, -1, s[..., 0:2], s[..., 2:4], ONES)
    with np.errstate(invalid="ignore"):
        f, _, _ = compose(lens, ONES, Wk, Hk, ns, eye, origin, wpm, info["entrance_pupil_z_mm"], info["exposure"],
                          tracer_samples(t, False, (len(pix), ns)), 6, emitter, [], [])
    ref = np.zeros((Hk, Wk, 3))
    ref[ys.reshape(-1), xs.reshape(-1)] = f
    want = centroid(ref)
    tol = 2.0 * max(abs(want[0] - pred[0]), abs(want[1] - pred[1])) + 0.1
    print(f"squeeze: chief ray predicts pixel {pred[0]:.3f}, {pred[1]:.3f}; float64-composed centroid {want[0]:.3f}, {want[1]:.3f}; "
          f"device {got[0]:.3f}, {got[1]:.3f}; tolerance {tol:.3f} px; {int(lit.sum())} lit pixels")
    assert abs(got[0] - pred[0]) <= tol and abs(got[1] - pred[1]) <= tol
    # the same emitter through the lens of spheres: no squeeze
    setup_scene_frame(pkg, lf, plain, ONES, Wk, Hk, ns, eye, origin, spheres=emitter, tris=[], lights=[])
    lf.set_lens_camera(1, wpm, 0.0)
    lf.render_scene_term()
    sph = centroid(lf.read_buffer(pkg.SCENE_BUFFER))
    ax, ay = got[0] - 0.5 * Wk, got[1] - 0.5 * Hk
    bx, by = sph[0] - 0.5 * Wk, sph[1] - 0.5 * Hk
    ratio = (ax / ay) / (bx / by)
    rel = tol * (1 / abs(ax) + 1 / abs(ay) + 1 / abs(bx) + 1 / abs(by))
    print(f"  offsets from the centre: anamorphic {ax:.3f}, {ay:.3f}; spherical {bx:.3f}, {by:.3f} px; ratio of x : y ratios "
          f"{ratio:.4f}, meridian scales {sx:.3f} : {sy:.3f} = {sx / sy:.4f}; relative tolerance {rel:.3f}")
    assert abs(sx / sy - 0.7495) < 1e-3                         # (37.744 mm : 50.358 mm)
    assert abs(ratio - sx / sy) <= rel * (sx / sy)


# ---- 5. exposure and aim --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_name", ["pentagon", "smooth"])
@pytest.mark.parametrize("name", ["asph", "anam"])
def test_calibrated_exposure_against_the_tracer(pkg, lf, pentagon, name, mask_name):
    """test_gpu_lens_camera_variants.test_calibrated_exposure_against_the_tracer on the recorded lenses: 4096 / the tracer's
    summed on-axis weights over the 64 x 64 cell centres of the pupil square, within W_TOL"""
    mask = pentagon if mask_name == "pentagon" else np.random.default_rng(20261019).uniform(0.25, 1.0, (16, 16)).astype(np.float32)
    lens = lens_of(name)
    setup_scene_frame(pkg, lf, lens, mask, W, H, NS, C2W, POS)
    lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_ALL)
    lf.set_lens_camera(1, WPM, 0.0)
    got = lf.lens_camera()["exposure"]
    g = (np.float32(2.0) * (np.arange(64, dtype=np.float32) + np.float32(0.5))) / np.float32(64.0) - np.float32(1.0)
    uv = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)
    t = br.trace_path(lens, 1, -1, -1, np.zeros_like(uv), uv, mask)
    want = 4096.0 / t[0][:, 6].sum()
    print(f"exposure {name} {mask_name}: device {got:.9g}, tracer {want:.9g}, relative {abs(got / want - 1.0):.2e}")
    assert abs(got - want) <= W_TOL * want


def test_aiming_at_the_exit_pupil_keeps_the_flat_field(pkg, lf, pentagon):
    """lf_set_lens_camera_aim(1.3) on the aspheric lens: the camera inside a uniformly bright sphere renders 1 on the axis
    again -- the calibration follows the lens camera's own disc (test_aiming_the_lens_camera_at_the_exit_pupil's flat field;
    the bar of test_closed_stop_converges_to_the_reference_pinhole_frames' centre, 64 samples a pixel) -- with more of the
    samples leaving the lens."""
    Wk, Hk, ns = 96, 64, 64
    lens = lens_of("asph")
    eye, origin = np.eye(3).reshape(-1), [0.0, 0.0, 0.0]
    glow = [(0.0, 0.0, 0.0, 50.0, "e", 1.0, 1.0, 1.0)]
    setup_scene_frame(pkg, lf, lens, pentagon, Wk, Hk, ns, eye, origin, spheres=glow, tris=[], lights=[])
    lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_ALL)
    lf.set_lens_camera(1, 0.001, 0.0)
    centres, left = [], []
    for margin in (0.0, 1.3):
        lf.set_lens_camera_aim(margin)
        lf.reset_scene_counters()
        lf.render_scene_term()
        flat = lf.read_buffer(pkg.SCENE_BUFFER)[..., 0] * (ns + 1) / ns
        centres.append(float(flat[Hk // 2 - 6:Hk // 2 + 6, Wk // 2 - 6:Wk // 2 + 6].mean()))
        left.append(lf.scene_counters()["lens_left"])
    print(f"flat field at the centre: {centres[0]:.4f} at the march's disc, {centres[1]:.4f} aimed at the exit pupil; "
          f"{left[1] / left[0]:.2f} x the samples leave")
    assert abs(centres[0] - 1.0) < 0.04 and abs(centres[1] - 1.0) < 0.04
    assert left[1] > 1.2 * left[0]


# ---- 6. nothing else moves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_a_lens_of_spheres_renders_the_same_bits(pkg, lf, pentagon, mode):
    """dgauss11.lens under ALL, and a context whose records were set and cleared again: the frame and the scene counters of the
    default setting, bit for bit"""
    plain, asph, anam = lens_of("plain"), lens_of("asph"), lens_of("anam")
    frames = []
    for how in ("default", "all", "danced"):
        setup_scene_frame(pkg, lf, plain, pentagon, W, H, NS, C2W, POS)
        lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_SPHERICAL if how == "default" else pkg.LENSCAM_SURFACES_ALL)
        if how == "danced":
            lf.set_lens_aspheres(asph["aspheres"]["conic"], asph["aspheres"]["coef"])
            lf.set_lens_camera(mode, WPM, 0.0)
            lf.render_scene_term()                              # (the records' table is built and used ...)
            lf.set_lens_aspheres(None)                          # (... and the lens is one of spheres again)
            assert lf.lens_aspheres()["n_aspheric"] == 0
        lf.set_lens_camera(mode, WPM, 0.0)
        lf.reset_scene_counters()
        lf.render_scene_term()
        frames.append((lf.read_buffer(pkg.SCENE_BUFFER), lf.scene_counters(), lf.lens_camera()))
    assert frames[0][0].max() > 0.02
    for k in (1, 2):
        assert np.array_equal(frames[0][0], frames[k][0]) and frames[0][1] == frames[k][1] and frames[0][2] == frames[k][2], k
    del anam


def test_setting_routing_and_the_row_deal(pkg, lf, pentagon):
    lens = lens_of("anam")
    setup_scene_frame(pkg, lf, lens, pentagon, W, H, NS, C2W, POS)
    # setter and getter; an invalid value
    assert lf.lens_camera_surfaces() == pkg.LENSCAM_SURFACES_SPHERICAL == 0 and pkg.LENSCAM_SURFACES_ALL == 1
    for bad in (2, -1):
        with pytest.raises(pkg.LensFlareError) as e:
            lf.set_lens_camera_surfaces(bad)
        assert e.value.status == LF_ERR_INVALID
    assert lf.lens_camera_surfaces() == pkg.LENSCAM_SURFACES_SPHERICAL
    # the default keeps the refusal (tests/test_gpu_biconics.py::test_routing holds its text)
    lf.set_lens_camera(1, WPM, 0.0)
    with pytest.raises(pkg.LensFlareError) as e:
        lf.render_scene_term()
    assert e.value.status == LF_ERR_UNSUPPORTED
    lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_ALL)
    assert lf.lens_camera_surfaces() == pkg.LENSCAM_SURFACES_ALL
    lf.render_scene_term()
    whole = lf.read_buffer(pkg.SCENE_BUFFER)
    assert whole.max() > 0.02
    # the per-lane kernel has no instantiation for records
    try:
        lf.test_knob("scene_compact", 0)
        with pytest.raises(pkg.LensFlareError) as e:
            lf.render_scene_term()
        assert e.value.status == LF_ERR_UNSUPPORTED and "scene_compact" in str(e.value)
    finally:
        lf.test_knob("scene_compact", -1)
    # rank 1 of 2 renders exactly its tile rows of the same frame
    lf.set_scene_term(np.zeros((H, W, 3)))
    lf.set_row_interleave(1, 2)
    lf.render_scene_term()
    part = lf.read_buffer(pkg.SCENE_BUFFER)
    lf.set_row_interleave(0, 1)
    own = (np.arange(H) // 8) % 2 == 1
    assert np.array_equal(part[own], whole[own]) and not part[~own].any()
    # back to the default: the refusal again
    lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_SPHERICAL)
    with pytest.raises(pkg.LensFlareError) as e:
        lf.lens_camera()
    assert e.value.status == LF_ERR_UNSUPPORTED and "biconic" in str(e.value)
    lf.set_lens_camera(0)
    assert math.isfinite(lf.lens_camera()["exposure"])
