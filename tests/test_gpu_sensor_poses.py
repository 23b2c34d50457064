"""Sensor ghosts through decentred and tilted lenses on the device (lf_set_sensor_ghost_surfaces(LF_SENSOR_SURFACES_POSED);
lens-flare_amd/csrc/lf_march_sensor.hip: k_march_sensor<VAR, 3>, k_march_sensor_path_rays<.., 3>): the per-ray query on
data/dgauss11_decentred.lens and on one posed face between spheres against the float64 tracer of tests/sensor_pose_ref.py, the
bit-for-bit identities -- zero records against the sphere-as-biconic twin, the frame as the composition of its own rays, ADD
as a sum, sums over interfaces and lights, deals, occlusion -- the routing and the setting.  Frames of 128 x 64 at 16 spp.
Every test here needs lf_set_sensor_ghost_surfaces: none passes on a library without it."""
import os

import numpy as np
import pytest

from goldenlib import load_texels

import asphere_ref as ar
import sensor_ghost_ref as sg
import sensor_pose_ref as sp
import test_sensor_poses_cpu as tc
from test_area_ghosts_cpu import RECTS, AREA, geom_of
from test_aspheres_cpu import COS_MIN
from test_gpu_sensor_ghosts import yardstick  # noqa: F401  (the fixture: D and Dw exactly as that file takes them)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "lens-flare_amd", "data")
MASK = "pentbig500_14.png"
W, H, SPP, KEY = 128, 64, 16, 0xA5F
SUN = (0, [0.012, 0.004, -1.0], [0.5, 1.0, 0.125], 0.03)
LAMP = (1, [1.5, -1.0, -90.0], [0.25, 0.125, 1.0], 0.05)
PANEL = (AREA, geom_of(RECTS[0]), [1.0, 0.5, 0.25], 0.0)
LIGHTS = (SUN, LAMP, PANEL)
LAMBDA_RGB = np.array([[0.5, 0.25, 0.0], [0.25, 0.5, 0.25], [0.0, 0.25, 0.5]], np.float32)
LF_ERR_INVALID, LF_ERR_UNSUPPORTED = 1, 6
OLD_FRAME_TEXT = "are not marched through a lens with posed interfaces (lf_set_lens_poses)"
OLD_RAYS_TEXT = "lf_march_sensor_path_rays: sensor paths are not marched through a lens with posed interfaces (lf_set_lens_poses)"


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="module")
def mask():
    return load_texels(MASK)


@pytest.fixture(scope="module")
def lf(pkg):
    ctx = pkg.LensFlare(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def plain(pkg):
    return pkg.load_lens_file("dgauss11.lens")


@pytest.fixture(scope="module")
def posed(pkg):
    return pkg.load_lens_file(tc.POSED)


def _with_poses(lens, records):
    """`lens` with pose records {k: (decentre, tilt_deg)}"""
    n = int(lens["n"])
    on = np.zeros(n, np.int32); t = np.zeros((n, 3), np.float32); a = np.zeros((n, 3), np.float32)
    for k, (dec, tilt) in records.items():
        on[k] = 1; t[k] = dec; a[k] = tilt
    out = dict(lens)
    out["poses"] = dict(on=on, decentre=t, tilt_deg=a)
    return out


def _setup(pkg, ctx, lens, mask, lights=LIGHTS, refl=0.5, mode=None, surfaces=None):
    ctx.set_frame(W, H)
    ctx.set_aperture(pkg.APERTURE_STARBURST, mask)
    ctx.set_lens(lens)
    ctx.set_lambda_rgb(LAMBDA_RGB)
    ctx.set_ghost_pairs(None, True)
    ctx.set_band(0, H)
    ctx.set_block_deal(0, 1)
    ctx.set_row_interleave(0, 1)
    ctx.set_mask_filter(pkg.MASK_NEAREST)
    ctx.set_ghost_accumulate(False)
    ctx.set_ghost_occlusion(False)
    ctx.set_march_culling(1)
    ctx.set_pupil_target(0.0, 0.0)
    ctx.set_lights_geom([l[0] for l in lights], [l[1] for l in lights], [l[2] for l in lights], [l[3] for l in lights])
    if refl is not None:
        ctx.set_sensor_reflectance(np.full(3, refl, np.float32) if np.isscalar(refl) else refl)
    ctx.set_sensor_ghosts(pkg.SENSOR_GHOSTS_OFF if mode is None else mode)
    ctx.set_sensor_ghost_surfaces(pkg.SENSOR_SURFACES_POSED if surfaces is None else surfaces)


def _frame(pkg, ctx, spp=SPP, key=KEY):
    ctx.reset_counters()
    ctx.trace_ghosts(spp, key)
    return ctx.read_buffer(pkg.GHOST_BUFFER).copy(), ctx.counters()


# ---- 1, 2. rays against float64 -------------------------------------------------------------------------------------------
def _compare(pkg, lf, T, yardstick, films, paths=None, refl=0.5):
    """lf_march_sensor_path_rays against T's float64 traces: alive / dead equal outside the exclusions, exit point and
    direction within 4 D n_ev, the weight within 4 Dw.  Returns (left out, cases, rays compared alive per path)."""
    D, Dw = yardstick["D"], yardstick["Dw"][films]
    lens = dict(T["lens"])
    if films:
        lens["coatings"] = yardstick["coat"]
    _setup(pkg, lf, lens, yardstick["open_mask"], (SUN,), refl=refl)
    n = int(lens["n"])
    left = total = 0
    worst = dict(pos=0.0, dir=0.0, w=0.0)
    compared = {}
    for i, t in T["paths"].items():
        if paths is not None and i not in paths:
            continue
        ref, cmin, rim, done, wb, edge, towards = t
        wref = (ref[:, 6] if films else wb) * refl
        bar = 4 * D * (3 * n - 2 * i)
        got = lf.march_sensor_path_rays(1, i, T["xy"], T["uv"])
        skip = sp.left_out(cmin, rim, edge, towards, bar, COS_MIN)
        left += int(skip.sum()); total += len(skip)
        keep = ~skip
        assert np.array_equal(got[keep, 7] == 1, ref[keep, 7] == 1), i
        a = keep & (ref[:, 7] == 1)
        compared[i] = int(a.sum())
        if a.any():
            worst["pos"] = max(worst["pos"], float(np.max(np.abs(got[a, 0:3] - ref[a, 0:3])) / bar))
            worst["dir"] = max(worst["dir"], float(np.max(np.abs(got[a, 3:6] - ref[a, 3:6])) / bar))
            worst["w"] = max(worst["w"], float(np.max(np.abs(got[a, 6] - wref[a]) / wref[a]) / (4 * Dw)))
    print(f"films {films}: D = {D:.3e}, Dw = {Dw:.3e}; worst deviation / bar: {worst}; left out {left} of {total}; compared {compared}")
    assert worst["pos"] <= 1.0 and worst["dir"] <= 1.0 and worst["w"] <= 1.0, worst
    return left, total, compared


@pytest.mark.parametrize("films", [False, True])
def test_rays_against_float64(pkg, lf, posed, yardstick, films):
    """every sensor path of dgauss11_decentred.lens over the 588-ray grid, bare and with dgauss11_coated.lens's films; at most
    2 % left out"""
    T = tc.traced(pkg, posed, tc.POSED)
    left, total, compared = _compare(pkg, lf, T, yardstick, films)
    assert total == 588 * 10 and left <= 0.02 * total
    assert sum(compared.values()) >= 300 and min(compared.values()) >= 5, compared


def test_one_posed_face_between_spheres(pkg, lf, plain, yardstick):
    """dgauss11.lens with ONE record, interface 9 tilted by 2 degrees and decentred by 0.1 mm, between spherical neighbours:
    the path whose mirror is the posed face, two whose mirror lies in front of it (the face is crossed three times; the stop
    and the spheres 6 .. 8 and 10 take a ray that comes out of a posed row) and the one whose mirror lies behind it (the face
    is crossed once, after the sensor's mirror) -- r2 must be the lens-frame one in front of every one of them"""
    lens = _with_poses(plain, {9: ((0.1, 0.0, 0.0), (2.0, 0.0, 0.0))})
    xy, uv = ar.comparison_grid()
    hw, hh = sg.rectangle(W, H, lens["sensor_width_mm"])
    paths = (9, 6, 2, 10)
    T = dict(lens=lens, xy=xy, uv=uv,
             paths={i: sp.trace_sensor_path(lens, 1, i, xy, uv, hw, hh, 1.0, None, yardstick["coat"]) for i in paths})
    left, total, compared = _compare(pkg, lf, T, yardstick, False)
    assert len(compared) >= 4 and min(compared.values()) >= 5, compared
    # ... and the record matters on each of them: the centred lens's rays are many bars away
    lf.set_lens_poses(None)
    for i in paths:
        ref = T["paths"][i][0]
        got = lf.march_sensor_path_rays(1, i, xy, uv)
        both = (got[:, 7] == 1) & (ref[:, 7] == 1)
        assert np.max(np.abs(got[both, 0:3] - ref[both, 0:3])) > 10 * 4 * yardstick["D"] * (33 - 2 * i), i


# ---- 3. identities, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stacks", [False, True])
def test_zero_records_are_the_sphere_as_biconic_twin(pkg, lf, plain, mask, stacks):
    """(stacks: with dgauss11_multicoated.lens's coating stacks -- the pose block then lies behind stack records)
    records of zeros on interfaces 1, 4 and 8 under POSED (k_march_sensor<.., 3>, pose_event with R = 1, t = 0) against the
    same lens with sphere-as-biconic records on those interfaces (the existing SURF = 2): the ONLY frame, the per-ray query
    and lf_get_sensor_ghost_stats"""
    ks = (1, 4, 8)
    if stacks:
        plain = dict(plain, coating_stacks=pkg.load_lens_file("dgauss11_multicoated.lens")["coating_stacks"])
    zero = _with_poses(plain, {k: ((0, 0, 0), (0, 0, 0)) for k in ks})
    n = int(plain["n"])
    on = np.zeros(n, np.int32); on[list(ks)] = 1
    rx = np.where(on != 0, np.asarray(plain["radius"], np.float32), np.float32(0)).astype(np.float32)
    twin = dict(plain)
    twin["biconics"] = dict(on=on, radius_x=rx, conic_x=np.zeros(n, np.float32), conic_y=np.zeros(n, np.float32))
    xy, uv = ar.comparison_grid()
    got = []
    lf.timing_enable(True)
    try:
        for lens in (zero, twin):
            _setup(pkg, lf, lens, mask, mode=pkg.SENSOR_GHOSTS_ONLY)
            lf.timing_reset()
            f, c = _frame(pkg, lf)
            assert lf.timing_get("march_sensor")[0] == 1
            lf.set_aperture(pkg.APERTURE_STARBURST, np.ones((64, 64), np.float32))          # (an open stop for the grid's rays)
            rays = [lf.march_sensor_path_rays(l, i, xy, uv) for i in (0, 4, 6, 10) for l in (0, 2)]
            got.append((f, lf.sensor_ghost_stats(), rays))
    finally:
        lf.timing_enable(False)
    assert got[0][0].max() > 0 and np.array_equal(got[0][0], got[1][0])
    assert got[0][1] == got[1][1] and got[0][1]["lit"] > 0
    for a, b in zip(got[0][2], got[1][2]):          # (a dead ray's NaNs may differ in their sign bit: the live rays bit for bit)
        live = a[:, 7] == 1
        assert np.array_equal(a[:, 6:8].view(np.uint32), b[:, 6:8].view(np.uint32)) and np.array_equal(np.isnan(a), np.isnan(b))
        assert np.array_equal(a[live].view(np.uint32), b[live].view(np.uint32))
    assert sum(int((a[:, 7] == 1).sum()) for a in got[0][2]) > 20


def test_the_frame_is_its_rays(pkg, lf, posed, mask):
    """_ONLY on dgauss11_decentred.lens under POSED: the device's samples (lf_lens_camera_samples, ns_aa = 16) through
    march_sensor_path_rays, ghost_ray_light_factors of the exit rays, composed in float32 as lights_epilogue does and summed
    as integers on the 2^36 grid (tests/test_gpu_sensor_ghosts.py does this for the centred lens): the ghost buffer bit for
    bit, the lit count the kernel's"""
    _setup(pkg, lf, posed, mask, refl=[0.5, 0.25, 0.125], mode=pkg.SENSOR_GHOSTS_ONLY)
    lf.set_params(ns_aa=SPP)
    lf.set_jitter_counter(KEY)
    img, _ = _frame(pkg, lf)
    stats = lf.sensor_ghost_stats()
    s = lf.lens_camera_samples(np.arange(W * H)).reshape(-1, 4)
    acc = np.zeros((W * H * SPP, 3), np.int64)
    lit = 0
    for i in tc.interfaces(posed):
        for l in range(3):
            out = lf.march_sensor_path_rays(l, i, s[:, 0:2], s[:, 2:4])
            live = np.flatnonzero(out[:, 7] == 1)
            if not len(live):
                continue
            fac = lf.ghost_ray_light_factors(out[live, :6])
            for k, light in enumerate(LIGHTS):
                contrib = (out[live, 6] * fac[:, k]).astype(np.float32)
                contrib = np.where(contrib > 0, contrib, np.float32(0))
                lit += int((contrib > 0).sum())
                for c in range(3):
                    ch = np.float32(np.float32(light[2][c]) * LAMBDA_RGB[l, c])
                    v = (contrib * ch).astype(np.float32) * np.float32(68719476736.0)
                    acc[live, c] += v.astype(np.int64)
    want = (acc.reshape(W * H, SPP, 3).sum(axis=1).astype(np.float64) * (1.0 / 68719476736.0)) / float(SPP)
    assert stats["lit"] == lit and lit > 100
    assert np.array_equal(img.reshape(-1, 3), want)


@pytest.mark.parametrize("spp", [16, 128])
def test_add_is_the_sum(pkg, lf, posed, mask, spp):
    _setup(pkg, lf, posed, mask)
    ordinary, c_ord = _frame(pkg, lf, spp)
    ev, ms = lf.executed_events(), lf.march_stats()
    assert lf.cull_reason() == "posed"
    lf.set_sensor_ghosts(pkg.SENSOR_GHOSTS_ONLY)
    only, _ = _frame(pkg, lf, spp)
    s_only = lf.sensor_ghost_stats()
    lf.set_sensor_ghosts(pkg.SENSOR_GHOSTS_ADD)
    both, c_add = _frame(pkg, lf, spp)
    s_add = lf.sensor_ghost_stats()
    assert only.max() > 0 and ordinary.max() > 0
    assert np.array_equal(both, np.add(ordinary, only))
    assert c_add == c_ord and lf.cull_reason() == "posed" and lf.executed_events() == ev and lf.march_stats() == ms
    assert s_add == s_only and s_add["started"] == W * H * spp * 10 * 3
    assert s_add["started"] >= s_add["reached_sensor"] >= s_add["lost_at_sensor"] and s_add["reached_sensor"] > 0 and s_add["lit"] > 0


def test_the_frame_is_the_sum_of_its_interfaces_and_of_its_lights(pkg, lf, posed, mask):
    _setup(pkg, lf, posed, mask, mode=pkg.SENSOR_GHOSTS_ONLY)
    whole, _ = _frame(pkg, lf)
    assert whole.max() > 0
    for n, i in enumerate(tc.interfaces(posed)):
        lf.set_sensor_ghosts(pkg.SENSOR_GHOSTS_ONLY, [i])
        lf.set_ghost_accumulate(n > 0)
        lf.trace_ghosts(SPP, KEY)
    summed = lf.read_buffer(pkg.GHOST_BUFFER).copy()
    lf.set_ghost_accumulate(False)
    assert np.array_equal(summed, whole)
    total = np.zeros_like(whole)
    for l in LIGHTS:
        _setup(pkg, lf, posed, mask, [l], mode=pkg.SENSOR_GHOSTS_ONLY)
        total += _frame(pkg, lf)[0]
    assert np.array_equal(total, whole)


def test_two_contexts_reproduce_the_add_frame_by_rows_and_by_blocks(pkg, lf, posed, mask):
    _setup(pkg, lf, posed, mask, [SUN, LAMP], mode=pkg.SENSOR_GHOSTS_ADD)
    whole, _ = _frame(pkg, lf)
    s_whole = lf.sensor_ghost_stats()
    others = [pkg.LensFlare(0), pkg.LensFlare(0)]
    try:
        for deal in ("rows", "blocks"):
            parts, ss = [], []
            for r, ctx in enumerate(others):
                _setup(pkg, ctx, posed, mask, [SUN, LAMP], mode=pkg.SENSOR_GHOSTS_ADD)
                if deal == "rows":
                    ctx.set_row_interleave(r, 2)
                else:
                    ctx.set_block_deal(r, 2)
                parts.append(_frame(pkg, ctx)[0]); ss.append(ctx.sensor_ghost_stats())
            yy, xx = np.mgrid[0:H, 0:W]
            own0 = ((yy >> 3) % 2 == 0) if deal == "rows" else (((yy >> 6) * ((W + 63) >> 6) + (xx >> 6)) % 2 == 0)
            assert np.array_equal(np.where(own0[..., None], parts[0], parts[1]), whole), deal
            for name in s_whole:
                assert ss[0][name] + ss[1][name] == s_whole[name], (deal, name)
    finally:
        for ctx in others:
            ctx.close()
    assert whole.max() > 0 and s_whole["lit"] > 0


@pytest.mark.parametrize("reach", ["SKY", "LIGHT"])
def test_occlusion_with_nothing_in_the_way_changes_no_bit(pkg, lf, posed, mask, reach):
    lights = [SUN] if reach == "SKY" else list(LIGHTS)          # (a point light needs the reach that ends at it)
    _setup(pkg, lf, posed, mask, lights, mode=pkg.SENSOR_GHOSTS_ONLY)
    lf.set_camera(np.eye(3).reshape(-1), [0.0, 0.0, 0.0], 40.0, 27.0)
    off, _ = _frame(pkg, lf)
    s_off = lf.sensor_ghost_stats()
    lf.set_scene([(0.0, 0.0, 50.0, 1.0, "d", 0.5, 0.5, 0.5)], [], [])      # a ball BEHIND the camera
    lf.set_ghost_occlusion_reach(getattr(pkg, "OCCLUSION_REACH_" + reach))
    lf.set_ghost_occlusion(True, 0.001)
    try:
        on, _ = _frame(pkg, lf)
        stats = lf.ghost_occlusion_stats()
        assert np.array_equal(on, off) and off.max() > 0 and lf.sensor_ghost_stats() == s_off
        assert stats["tested"] > 0 and stats["blocked"] == 0
    finally:
        lf.set_ghost_occlusion(False)
        lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_SKY)


# ---- 4. routing -----------------------------------------------------------------------------------------------------------
def test_refusals_under_centred_and_the_launch_under_posed(pkg, lf, posed, mask):
    _setup(pkg, lf, posed, mask, surfaces=pkg.SENSOR_SURFACES_CENTRED)
    for mode in (pkg.SENSOR_GHOSTS_ADD, pkg.SENSOR_GHOSTS_ONLY):
        lf.set_sensor_ghosts(mode)
        with pytest.raises(pkg.LensFlareError) as e:
            lf.trace_ghosts(SPP, KEY)
        assert e.value.status == LF_ERR_UNSUPPORTED and OLD_FRAME_TEXT in str(e.value) and "lf_set_sensor_ghost_surfaces" in str(e.value)
        assert "lf_set_sensor_ghosts" in str(e.value)
    with pytest.raises(pkg.LensFlareError) as e:
        lf.march_sensor_path_rays(1, 2, np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32))
    assert e.value.status == LF_ERR_UNSUPPORTED and OLD_RAYS_TEXT in str(e.value) and "lf_set_sensor_ghost_surfaces" in str(e.value)
    lf.set_sensor_ghost_surfaces(pkg.SENSOR_SURFACES_POSED)
    lf.timing_enable(True)
    try:
        for mode, n_march in ((pkg.SENSOR_GHOSTS_ADD, 1), (pkg.SENSOR_GHOSTS_ONLY, 0)):
            lf.set_sensor_ghosts(mode)
            lf.timing_reset()
            f, _ = _frame(pkg, lf)
            assert f.max() > 0 and lf.timing_get("march_sensor")[0] == 1 and lf.timing_get("march")[0] == n_march
        # an unchanged frame uploads no table; a change of ONE pose record uploads one and changes the frame
        lf.timing_reset()
        again, _ = _frame(pkg, lf)
        assert np.array_equal(again, f) and lf.timing_get("sensor_table")[0] == 0 and lf.timing_get("march_sensor")[0] == 1
        p = posed["poses"]
        t = np.array(p["decentre"], np.float32).copy(); t[3, 0] += np.float32(0.05)
        lf.set_lens_poses(p["on"], t, p["tilt_deg"])
        lf.timing_reset()
        moved, _ = _frame(pkg, lf)
        assert lf.timing_get("sensor_table")[0] == 1 and not np.array_equal(moved, f)
        lf.set_lens_poses(p["on"], p["decentre"], p["tilt_deg"])
        lf.timing_reset()
        back, _ = _frame(pkg, lf)
        assert lf.timing_get("sensor_table")[0] == 1 and np.array_equal(back, f)
    finally:
        lf.timing_enable(False)


def test_a_lens_without_poses_is_what_it_was(pkg, lf, mask):
    """dgauss11_sensor.lens: the ONLY and ADD frames, the stats, the counters and the launch counts under POSED are those
    under CENTRED, and a second identical frame uploads no table"""
    lens = pkg.load_lens_file("dgauss11_sensor.lens")
    got = {}
    lf.timing_enable(True)
    try:
        for which in (pkg.SENSOR_SURFACES_CENTRED, pkg.SENSOR_SURFACES_POSED):
            for mode in (pkg.SENSOR_GHOSTS_ONLY, pkg.SENSOR_GHOSTS_ADD):
                _setup(pkg, lf, lens, mask, refl=None, mode=mode, surfaces=which)
                lf.timing_reset()
                f, c = _frame(pkg, lf)
                counts = {k: lf.timing_get(k)[0] for k in ("march", "march_sensor", "cull_prepass")}
                lf.timing_reset()
                f2, _ = _frame(pkg, lf)
                assert np.array_equal(f2, f) and lf.timing_get("sensor_table")[0] == 0
                reason = lf.cull_reason() if mode == pkg.SENSOR_GHOSTS_ADD else None          # (ONLY runs no ordinary march)
                got[which, mode] = (f, c, lf.sensor_ghost_stats(), reason, counts)
    finally:
        lf.timing_enable(False)
    for mode in (pkg.SENSOR_GHOSTS_ONLY, pkg.SENSOR_GHOSTS_ADD):
        a, b = got[pkg.SENSOR_SURFACES_CENTRED, mode], got[pkg.SENSOR_SURFACES_POSED, mode]
        assert a[0].max() > 0 and np.array_equal(a[0], b[0]) and a[1:] == b[1:], mode


def test_a_lens_file_with_pose_and_reflectance_lines(pkg, lf, mask, tmp_path):
    src = open(os.path.join(DATA, "dgauss11.lens")).read()
    path = tmp_path / "posed_sensor.lens"
    path.write_text(src + "pose 9 0.1 0 0 2 0 0\npose 3 0 -0.05 0 0 1 45\nsensor_reflectance 0.05 0.1 0.2\n")
    lens = pkg.load_lens_file(str(path))
    assert lens["poses"]["on"].sum() == 2 and np.array_equal(lens["sensor_reflectance"], np.array([0.05, 0.1, 0.2], np.float32))
    _setup(pkg, lf, lens, mask, refl=None, mode=pkg.SENSOR_GHOSTS_ONLY)
    py, _ = _frame(pkg, lf)
    lf.load_lens_file(str(path))                                   # the C parser
    g = lf.lens_poses()
    for key in ("on", "decentre", "tilt_deg"):
        assert np.array_equal(g[key], lens["poses"][key]), key
    assert np.array_equal(lf.sensor_reflectance(), lens["sensor_reflectance"])
    lf.set_lambda_rgb(LAMBDA_RGB)
    c, _ = _frame(pkg, lf)
    assert py.max() > 0 and np.array_equal(py, c)


# ---- 5. the setting -------------------------------------------------------------------------------------------------------
def test_the_setting(pkg, lf, plain, posed, mask):
    _setup(pkg, lf, plain, mask, surfaces=pkg.SENSOR_SURFACES_CENTRED)
    assert lf.sensor_ghost_surfaces() == pkg.SENSOR_SURFACES_CENTRED
    fresh = pkg.LensFlare(0)
    try:
        assert fresh.sensor_ghost_surfaces() == pkg.SENSOR_SURFACES_CENTRED          # the default
    finally:
        fresh.close()
    lf.set_sensor_ghost_surfaces(pkg.SENSOR_SURFACES_POSED)
    for bad in (2, 3, -1):
        with pytest.raises(pkg.LensFlareError) as e:
            lf.set_sensor_ghost_surfaces(bad)
        assert e.value.status == LF_ERR_INVALID and "LF_SENSOR_SURFACES_POSED" in str(e.value)
        assert lf.sensor_ghost_surfaces() == pkg.SENSOR_SURFACES_POSED               # a refusal leaves the state
    lf.set_lens(posed)                                                               # ... and so do lf_set_lens and lf_focus_lens
    lf.focus_lens(4000.0)
    assert lf.sensor_ghost_surfaces() == pkg.SENSOR_SURFACES_POSED
    lf.set_sensor_reflectance([0.5, 0.5, 0.5])
    out = lf.march_sensor_path_rays(1, 2, [[0.0, 0.0]], [[0.5, 0.5]])
    assert out.shape == (1, 8)
    lf.set_sensor_ghost_surfaces(pkg.SENSOR_SURFACES_CENTRED)
    with pytest.raises(pkg.LensFlareError) as e:
        lf.march_sensor_path_rays(1, 2, [[0.0, 0.0]], [[0.5, 0.5]])
    assert e.value.status == LF_ERR_UNSUPPORTED
