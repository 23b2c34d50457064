"""Flare occlusion on the device (lf_set_flare_occlusion; lens-flare_amd/csrc/lf_flare_occlusion.hip: k_flare_visibility,
k_flare_visibility_apply): the starburst, the falloff and the paraxial ghost quads of a flare scaled by the fraction of its
shadow rays the resident scene leaves free.

Every count is an integer and every effect one double multiply, so the identities are bit for bit; the one tolerance, the
paraxial ghost buffer against visibility x the unoccluded buffer, is derived where it is used.

A 64 x 48 frame, the double-Gauss prescription, the pentagon mask, the identity pose at the origin with a 40 x 27 degree
field of view, 0.001 scene units per lens millimetre and the sun's angular radius."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from goldenlib import load_texels
from test_flare_occlusion_cpu import (ALPHA, CAMERA, FLARES, FRONT, HFOV, VFOV, WPM, beam_centre_x, quad_margin, shadow_ray64)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "lens-flare_amd", "host", "shim_demo")
W, H = 64, 48
MASK = "pentbig500_14.png"
RAD, RAD2 = [1.0, 0.9, 0.5], [0.5, 1.0, 0.8]
LF_ERR_INVALID, LF_ERR_STATE = 1, 4
KEY = 0x1e45f1a4e
FAR_QUAD = (3.0, 3.1, 3.0, 3.1, 5.0)          # behind the camera and off to the side: outside every beam
EVERYTHING = (-5.0, 5.0, -5.0, 5.0, -0.8)     # a wall over the whole field of view


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="module")
def mask():
    return load_texels(MASK)


@pytest.fixture(scope="module")
def lens(pkg):
    return pkg.load_lens_file("dgauss11.lens")


@pytest.fixture(scope="module")
def lf(pkg, mask, lens):
    ctx = pkg.LensFlare(0)
    _frame_state(pkg, ctx, mask)
    ctx.set_lens(lens)
    yield ctx
    ctx.close()


def _frame_state(pkg, ctx, mask, width=W):
    ctx.set_frame(width, H)
    ctx.set_params(1, 20.0, 1.0)
    ctx.set_aperture(pkg.APERTURE_STARBURST, mask)
    ctx.set_aperture(pkg.APERTURE_GHOST, mask)
    ctx.set_jitter_counter(KEY)


def _camera(ctx):
    ctx.set_camera(np.eye(3).reshape(-1), [0.0, 0.0, 0.0], HFOV, VFOV)


def _quad(x0, x1, y0, y1, z):
    """two triangles over [x0, x1] x [y0, y1] of the world plane z, as set_scene's rows"""
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    n = (0.0, 0.0, 1.0)
    row = lambda p, q, r: tuple(p + q + r + n + n + n) + ("d", 0.5, 0.5, 0.5)      # noqa: E731
    return [row(a, b, c), row(a, c, d)]


def _flares(ctx, origins, radiance):
    o = np.asarray(origins, np.float64).reshape(-1, 2)
    ctx.set_flares(o, np.asarray(radiance, np.float64).reshape(-1, 3), o[-1], float(np.float32(np.arctan(o[-1, 1] / o[-1, 0]))))


def _z_ref(ctx):
    """the paraxial entrance pupil's z, as lf_get_lens_camera reports it"""
    ctx.set_lens_camera(1, WPM, 1.0)
    try:
        return ctx.lens_camera()["entrance_pupil_z_mm"]
    finally:
        ctx.set_lens_camera(0)


def _buffers(pkg, ctx, ghosts):
    """one frame: the paraxial quads (or an empty ghost buffer), then the flare layer -> buffers 0, 1, 2"""
    if ghosts:
        ctx.generate_ghost_buffer()
    else:
        ctx.clear_ghost_buffer()
    ctx.render_flare_layer()
    return [ctx.read_buffer(b) for b in (pkg.SAMPLE_BUFFER, pkg.GHOST_BUFFER, pkg.STARBURST_BUFFER)]


def _same(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _wall(flare, origin, z_ref):
    cx = beam_centre_x(flare, -0.8, origin, WPM, z_ref)
    return (cx - 0.5, cx + 0.0013, -0.6, 0.7, -0.8)


# ---- 1: the counts are the per-ray answers ------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [FRONT, CAMERA])
def test_counts_are_the_per_ray_answers(pkg, lf, lens, origin):
    _camera(lf)
    z_ref = _z_ref(lf)
    h0 = float(lens["semi_aperture"][0])
    lf.set_ghost_occlusion(True, WPM)       # (lf_ghost_ray_visibility takes its scale from it)
    try:
        for flare in FLARES:
            wall = _wall(flare, origin, z_ref)
            lf.set_scene(tris=_quad(*wall))
            _flares(lf, [flare], [RAD])
            right, wrong = [], dict(x_flipped=[], z_ref_dropped=[], wpm_squared=[])
            for R in (64, 256, 1024):
                lf.set_flare_occlusion(True, R, ALPHA, origin, WPM)
                fv = lf.flare_visibility()
                assert fv["n"] == 1
                got = int(fv["visible_rays"][0])
                assert fv["visibility"][0] == got / R
                rays = pkg.flare_shadow_rays(R, flare, HFOV, VFOV, ALPHA, origin, h0)
                # the float64 analytic ray-quad count, no ray left out, none fragile
                o, d = shadow_ray64(rays, WPM, z_ref) if origin == FRONT else shadow_ray64(rays, 1.0, 0.0)
                hit, margin = quad_margin(o, d, wall[4], *wall[:4])
                print(f"origin {origin} flare {flare} R {R}: visible {got}, analytic blocked {int(hit.sum())}, smallest margin {margin.min():.3e}")
                assert margin.min() >= 1e-9
                assert got == R - int(hit.sum())
                assert 0 < got < R
                # ... and the library's own per-ray answers
                if origin == FRONT:
                    assert got == int(lf.ghost_ray_visibility(rays).sum())
                    right.append(got)
                    for name, kw in (("x_flipped", dict(x_flip=-1.0)), ("z_ref_dropped", dict(use_z_ref=False)), ("wpm_squared", dict(wpm_power=2))):
                        wrong[name].append(R - int(quad_margin(*shadow_ray64(rays, WPM, z_ref, **kw), wall[4], *wall[:4])[0].sum()))
                else:
                    misses = sum(0 if lf.scene_trace_ray(o[i], d[i], seq=i)["hit"] else 1 for i in range(R))
                    assert got == misses
            if origin == FRONT and flare != FLARES[0]:      # (on the axis z_ref only moves the origin along the beam)
                for name, counts in wrong.items():
                    assert counts != right, (flare, name, right)
    finally:
        lf.set_ghost_occlusion(False)
        lf.set_flare_occlusion(False)


# ---- 2: nothing in the way ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", ["mt19937", "counter"])
def test_nothing_in_the_way_changes_no_bit(pkg, lf, jitter):
    _camera(lf)
    lf.set_scene(tris=_quad(*FAR_QUAD))
    if jitter == "mt19937":
        lf.set_jitter_mt19937(5489, None)
    try:
        for origins, rads in (([FLARES[1]], [RAD]), ([FLARES[2], FLARES[1]], [RAD2, RAD])):
            _flares(lf, origins, rads)
            lf.set_flare_occlusion(False)
            off = _buffers(pkg, lf, True)
            for origin in (CAMERA, FRONT):
                lf.set_flare_occlusion(True, 256, ALPHA, origin, WPM)
                fv = lf.flare_visibility()
                assert fv["n"] == len(origins) and (fv["visibility"] == 1.0).all() and (fv["visible_rays"] == 256).all()
                on = _buffers(pkg, lf, True)
                for b in range(3):
                    assert _same(on[b], off[b]), (jitter, len(origins), origin, b)
                assert off[1].max() > 0 and off[2].max() > 0
                px = lf.irradiance_falloff(20, 30, 5.0)
                lf.set_flare_occlusion(False)
                assert _same(px, lf.irradiance_falloff(20, 30, 5.0))
    finally:
        lf.set_flare_occlusion(False)
        lf.set_jitter_counter(KEY)


# ---- 3: fully hidden ------------------------------------------------------------------------------------------------------
def _hidden_frames(pkg, lf):
    """(on behind a wall over everything, off with the radiance set to zero), each with an empty ghost buffer"""
    _camera(lf)
    lf.set_scene(tris=_quad(*EVERYTHING))
    _flares(lf, [FLARES[1]], [RAD])
    lf.set_flare_occlusion(True, 1024, 0.05, CAMERA)
    on = _buffers(pkg, lf, False)
    fv = lf.flare_visibility()
    lf.set_flare_occlusion(False)
    _flares(lf, [FLARES[1]], [[0.0, 0.0, 0.0]])
    off = _buffers(pkg, lf, False)
    return on, off, fv


def test_fully_hidden_is_the_frame_of_a_dark_light(pkg, lf):
    try:
        on, off, fv = _hidden_frames(pkg, lf)
        assert fv["n"] == 1 and fv["visibility"][0] == 0.0 and fv["visible_rays"][0] == 0
        assert _same(on[0], off[0]) and _same(on[2], off[2])
        # ... and with its radiance back the same light is bright: the wall did that
        _flares(lf, [FLARES[1]], [RAD])
        assert _buffers(pkg, lf, False)[2].max() > 100 * max(on[2].max(), 1e-300)
        for origin in (CAMERA, FRONT):
            lf.set_flare_occlusion(True, 64, ALPHA, origin, WPM)
            lf.generate_ghost_buffer()
            assert not lf.read_buffer(pkg.GHOST_BUFFER).any()
        lf.set_flare_occlusion(False)
        lf.generate_ghost_buffer()
        assert lf.read_buffer(pkg.GHOST_BUFFER).max() > 0
    finally:
        lf.set_flare_occlusion(False)


# ---- 4: partly hidden, two flares ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [FRONT, CAMERA])
def test_partly_hidden_is_the_frame_of_the_scaled_radiance(pkg, lf, origin):
    _camera(lf)
    z_ref = _z_ref(lf)
    free, hidden = FLARES[1], FLARES[2]       # the hidden one last: it supplies axis_ray, the quads are its
    lf.set_scene(tris=_quad(*_wall(hidden, origin, z_ref)))
    rad = np.array([RAD2, RAD], np.float64)
    try:
        _flares(lf, [free, hidden], rad)
        lf.set_flare_occlusion(True, 1024, ALPHA, origin, WPM)
        on = _buffers(pkg, lf, False)
        fv = lf.flare_visibility()
        vis = fv["visibility"]
        assert fv["n"] == 2 and vis[0] == 1.0 and 0.0 < vis[1] < 1.0 and vis[1] == int(fv["visible_rays"][1]) / 1024
        got = lf.get_flares()
        assert got["n"] == 2 and _same(got["radiance"], rad)      # the radiance as installed
        px_on = lf.irradiance_falloff(40, 20, 5.0)
        ghost_on = _buffers(pkg, lf, True)[1]
        lf.set_flare_occlusion(False)
        ghost_off = _buffers(pkg, lf, True)[1]
        _flares(lf, [free, hidden], rad * vis[:, None])
        off = _buffers(pkg, lf, False)
        assert _same(on[0], off[0]) and _same(on[2], off[2])
        assert _same(px_on, lf.irradiance_falloff(40, 20, 5.0))
        # The quads: every term s * (colour * v) of a pixel's sum is non-negative and carries at most two roundings more
        # than v * (s * colour); fewer than 80 quads overlap in a pixel: below 80 * 2^-53 ~ 9e-15 relative, asked to 1e-13.
        lit = ghost_off > 0
        assert lit.any() and np.array_equal(ghost_on > 0, lit)
        rel = np.abs(ghost_on[lit] - vis[1] * ghost_off[lit]) / (vis[1] * ghost_off[lit])
        print(f"origin {origin}: visibility {vis[1]}, paraxial quads off by {rel.max():.3e} relative at most")
        assert rel.max() <= 1e-13
    finally:
        lf.set_flare_occlusion(False)


# ---- 5: state -----------------------------------------------------------------------------------------------------------
def test_the_library_refuses_what_the_contract_refuses_and_keeps_its_state(pkg, lf):
    lf.set_flare_occlusion(True, 256, ALPHA, FRONT, 0.002)
    try:
        before = lf.get_flare_occlusion()
        assert before == dict(on=True, rays_per_light=256, angular_radius=float(np.float32(ALPHA)), origin=FRONT, world_per_mm=0.002)
        call = lambda R, a, o, w: lf.lib.lf_set_flare_occlusion(lf.ctx, 1, C.c_int(R), C.c_float(a), C.c_int(o), C.c_double(w))      # noqa: E731
        for args in ((63, ALPHA, CAMERA, WPM), (65, ALPHA, CAMERA, WPM), (4160, ALPHA, CAMERA, WPM), (64, -1e-6, CAMERA, WPM),
                     (64, 0.5001, CAMERA, WPM), (64, float("nan"), CAMERA, WPM), (64, ALPHA, 2, WPM), (64, ALPHA, -1, WPM),
                     (64, ALPHA, FRONT, 0.0), (64, ALPHA, FRONT, -WPM), (64, ALPHA, FRONT, float("inf")), (64, ALPHA, FRONT, float("nan"))):
            assert call(*args) == LF_ERR_INVALID, args
            assert lf.get_flare_occlusion() == before, args
        # the limits themselves are fine; CAMERA ignores the scale and keeps the one installed
        assert call(4096, 0.5, CAMERA, -1.0) == 0
        assert lf.get_flare_occlusion() == dict(on=True, rays_per_light=4096, angular_radius=0.5, origin=CAMERA, world_per_mm=0.002)
        assert call(64, 0.0, FRONT, WPM) == 0
        # the setting survives the frame, the lens, the camera and both ways of installing flares
        now = lf.get_flare_occlusion()
        _camera(lf)
        lf.find_sun_pos([[0.0, 0.0, -1e6, 1.0, 1.0, 1.0]])
        _flares(lf, [FLARES[0]], [RAD])
        assert lf.get_flare_occlusion() == now
    finally:
        lf.set_flare_occlusion(False)
    assert lf.get_flare_occlusion()["on"] is False


def test_state_errors_name_what_is_missing(pkg, mask, lens):
    ctx = pkg.LensFlare(0)
    try:
        _frame_state(pkg, ctx, mask)
        _flares(ctx, [FLARES[1]], [RAD])
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.flare_visibility()                       # off: there is nothing to report
        assert e.value.status == LF_ERR_STATE
        ctx.set_flare_occlusion(True, 256, ALPHA, CAMERA)
        for call in (ctx.render_flare_layer, ctx.generate_ghost_buffer, ctx.flare_visibility, lambda: ctx.irradiance_falloff(3, 3, 5.0)):
            with pytest.raises(pkg.LensFlareError) as e:
                call()
            assert e.value.status == LF_ERR_STATE and "a camera" in str(e.value) and "a scene" in str(e.value) and "a lens" not in str(e.value)
        ctx.set_scene(tris=_quad(*EVERYTHING))
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.render_flare_layer()
        assert e.value.status == LF_ERR_STATE and "a camera" in str(e.value) and "a scene" not in str(e.value)
        _camera(ctx)
        # CAMERA needs no lens: it renders, and the wall hides the light
        hidden = _buffers(pkg, ctx, True)
        assert ctx.flare_visibility()["visibility"][0] == 0.0 and not hidden[1].any()
        ctx.set_flare_occlusion(True, 256, ALPHA, FRONT, WPM)
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.render_flare_layer()
        assert e.value.status == LF_ERR_STATE and "a lens" in str(e.value) and "a camera" not in str(e.value) and "a scene" not in str(e.value)
        ctx.set_lens(lens)
        again = _buffers(pkg, ctx, True)
        assert _same(again[2], hidden[2])
        # moving the wall between two frames changes the second: nothing stale is kept
        ctx.set_scene(tris=_quad(*FAR_QUAD))
        ctx.render_flare_layer()
        shown = ctx.read_buffer(pkg.STARBURST_BUFFER)
        assert ctx.flare_visibility()["visibility"][0] == 1.0
        assert shown.max() > 100 * max(hidden[2].max(), 1e-300) and not _same(shown, hidden[2])
        # no flare in the frame: nothing is launched, nothing fails
        ctx.timing_enable(True)
        ctx.timing_reset()
        ctx.set_flares(np.zeros((0, 2)), np.zeros((0, 3)), [0.5, 0.5], 0.0)
        ctx.render_flare_layer()
        assert ctx.flare_visibility()["n"] == 0
        assert ctx.timing_get("flare_visibility")[0] == 0
        # the timing entry counts consuming calls only while the setting is on
        _flares(ctx, [FLARES[1]], [RAD])
        ctx.set_flare_occlusion(False)
        ctx.generate_ghost_buffer()
        ctx.render_flare_layer()
        assert ctx.timing_get("flare_visibility")[0] == 0
        ctx.set_flare_occlusion(True, 256, ALPHA, FRONT, WPM)
        ctx.generate_ghost_buffer()
        ctx.render_flare_layer()
        n, ms = ctx.timing_get("flare_visibility")
        assert n == 2 and ms > 0.0
        assert ctx.timing_get("flare_layer")[0] == 3
    finally:
        ctx.close()


# ---- 6: ranks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [64, 128])
def test_two_ranks_count_the_same_and_gather_to_the_single_frame(pkg, mask, lens, width):
    z_ref = None
    frames, counts = [], []
    for rank, n in ((0, 1), (0, 2), (1, 2)):
        ctx = pkg.LensFlare(0)
        try:
            _frame_state(pkg, ctx, mask, width)
            ctx.set_lens(lens)
            _camera(ctx)
            z_ref = _z_ref(ctx) if z_ref is None else z_ref
            ctx.set_scene(tris=_quad(*_wall(FLARES[2], FRONT, z_ref)))
            _flares(ctx, [FLARES[1], FLARES[2]], [RAD2, RAD])
            ctx.set_block_deal(rank, n)
            ctx.set_flare_occlusion(True, 256, ALPHA, FRONT, WPM)
            frames.append(_buffers(pkg, ctx, True))
            counts.append(ctx.flare_visibility()["visible_rays"].tolist())
        finally:
            ctx.close()
    assert counts[0] == counts[1] == counts[2] and 0 < counts[0][1] < 256 and counts[0][0] == 256
    owner = ((np.arange(width) >> 6) % 2)[None, :, None] * np.ones((H, 1, 3), int)
    for b in range(3):
        assert _same(np.where(owner == 0, frames[1][b], frames[2][b]), frames[0][b]), b


# ---- 7: the host mirror -------------------------------------------------------------------------------------------------
def test_the_host_mirror_hides_the_sun_behind_the_wall(pkg, lf, mask, tmp_path):
    """shim_demo flarewall: lfamd::PathTracer::use_flare_occlusion -> lf_frame_plan::flare_occlusion -> lf_run_frame"""
    ap = tmp_path / "mask.f32"
    np.ascontiguousarray(mask, np.float32).tofile(ap)
    h, w = mask.shape
    run = subprocess.run([DEMO, "flarewall", str(ap), str(w), str(h), str(ap), str(w), str(h), str(W), str(H), str(HFOV), str(VFOV),
                          str(FLARES[1][0]), str(FLARES[1][1]), str(tmp_path / "out"), "1", "1024"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "flare 0 visibility 0 visible rays 0 of 1024" in run.stdout, run.stdout
    got = {name: np.fromfile(tmp_path / f"out.{name}.f64", np.float64).reshape(H, W, 3) for name in ("sample", "star", "ghost")}
    try:
        on, off, _ = _hidden_frames(pkg, lf)
    finally:
        lf.set_flare_occlusion(False)
    assert not got["ghost"].any()
    assert _same(got["star"], on[2]) and _same(got["star"], off[2])
    assert _same(got["sample"], on[0])
