"""Occluded ghost frames on the GPU against the INDEPENDENT float64 tracer (oracle/lf_geo_f64.c under an occluder list:
lfo.g64_trace(occlusion=...), anchored by tests/test_geo_f64_occlusion_cpu.py), at the bar tests/test_gpu_march_f64.py holds the
sun to: every lit value within 1e-4 relative, the fragile rays' weight the only allowance -- which now holds the occluders' edge
band too.  What the identities of tests/test_gpu_ghost_occlusion.py / test_gpu_near_occlusion.py cannot see -- every one of them
relates device frames that all go through the one lights_epilogue<VAR & kVarOccl> (lf_march_common.h) -- is seen here: the
lit value of an occluded frame against a tracer that maps, reaches and intersects in its own words, by brute force, each light on
its own.  Every frame stands under ONE GENERAL POSE (0.4 rad about (1, 2, 3), away from the origin): a transposed c2w is another
frame.  The occluders are written in camera coordinates and carried to the world by the test, in float64; the device and the
tracer are handed the same world numbers, the tracer its lights from ctx.lights_geom() and z_ref from ctx.lens_camera().

Each test prints the lit values, those needing the allowance, the largest raw deviation, the median, and (tested, blocked, edge)
pairs per light (record: profiles/occlusion_f64_parity.txt, with the five mutants built against this file)."""
import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo
from test_geo_f64_lights_cpu import MASK, AREA
from test_geo_f64_occlusion_cpu import OCCL_FRAMES, POSE, IDENTITY, WPM, EDGE_CAP, frame_of
from test_gpu_area_ghosts import _setup, _install, _frame
from test_gpu_march_f64 import _check_against_f64, TOL, FLOOR

pytestmark = pytest.mark.gpu
ROW = ("d", 0.5, 0.5, 0.5)
NORMAL = (0.0, 0.0, 1.0) * 3          # (an occluder is opaque whatever its shading normals are)


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


@pytest.fixture()
def forced(pkg, lf):
    """the culled march whatever the table starts, as tests/test_gpu_lights_f64.py forces it"""
    lf.test_knob("cull_force", 1)
    pkg.test_knob_default("cull_force", 1)
    yield
    lf.test_knob("cull_force", 0)
    pkg.test_knob_default("cull_force", 0)


def _z_ref(lf):
    """the paraxial entrance pupil's z, as lf_get_lens_camera reports it"""
    lf.set_lens_camera(1, WPM, 1.0)
    try:
        return lf.lens_camera()["entrance_pupil_z_mm"]
    finally:
        lf.set_lens_camera(0)


def _occluded_frame(pkg, lf, mask, name, spp, mode=0, bits=6, pose=POSE):
    """FRAMES[name] on the device under `pose`: -> (image, counters, stats, what frame_of returns)"""
    f = frame_of(pkg, name, pose)
    lens, W, H, key, lights, occlusion, partly, lambda_rgb, (sp, tr) = f
    _setup(pkg, lf, lens, W, H, mask, lambda_rgb if lambda_rgb is not None else np.eye(3))
    assert _z_ref(lf) == occlusion["z_ref_mm"]          # (the table's z_ref is the context's)
    lf.set_pupil_subcells(bits)
    _install(lf, lights)
    lf.set_camera(pose[0].reshape(-1), pose[1], 40.0, 27.0)
    lf.set_scene([tuple(s) + ROW for s in sp], [tuple(t) + NORMAL + ROW for t in tr], [])
    lf.set_ghost_occlusion(True, WPM)
    lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_LIGHT if occlusion["reach"] == lfo.REACH_LIGHT else pkg.OCCLUSION_REACH_SKY)
    img, cnt = _frame(pkg, lf, spp, key, mode)
    return img, cnt, lf.ghost_occlusion_stats(), f


def _restore(pkg, lf):
    lf.set_ghost_occlusion(False)
    lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_SKY)
    lf.set_camera(np.eye(3).reshape(-1), [0.0, 0.0, 0.0], 40.0, 27.0)
    lf.set_lambda_rgb(np.eye(3))
    lf.set_pupil_subcells(6)


def _against_f64(pkg, lf, mask, name, spp, mode=0, bits=6, label=None, min_lit=150, audit=False):
    try:
        img, cnt, stats, f = _occluded_frame(pkg, lf, mask, name, spp, mode, bits)
        culled = lf.cull_info()["culled"]
        if audit:          # the culled march ran, and its table dropped no lit ray
            assert culled, lf.cull_reason()
            found = lf.cull_audit()
            assert found["rays"] > 0 and found["lit"] == 0, found
        table = lf.cull_table_and_block()
        stored = lfo.lights_of(lf)
    finally:
        _restore(pkg, lf)
    lens, W, H, key, lights, occlusion, partly, lambda_rgb, _ = f
    assert [l[0] for l in stored] == [l[0] for l in lights]
    ref, frag, c64 = lfo.g64_trace(lens, W, H, 0, H, spp, key, None, True, mask, [0.0, 0.0, -1.0], [0.0, 0.0, 0.0], 0.05,
                                   n_threads=16, sub_bits=bits, cull=table, lights=stored, occlusion=occlusion, lambda_rgb=lambda_rgb)
    o = lfo.g64_last_occlusion_pairs
    per_light = o["per_light"][:len(lights)]
    lit = ref >= FLOOR
    dev = np.abs(img - ref)
    rel = dev[lit] / ref[lit]
    over = int((dev[lit] > TOL * ref[lit]).sum())
    print(f"{label or name}: {int(lit.sum())} lit values, {over} need the allowance, largest raw deviation {rel.max() if rel.size else 0:.2e}, "
          f"median {np.median(rel) if rel.size else 0:.2e}; per light (tested, blocked, edge) {per_light}; device tested {stats['tested']} "
          f"blocked {stats['blocked']} (float64 {o['tested']} / {o['blocked']}); rays_hit_light {cnt['rays_hit_light']} (float64 "
          f"{c64['rays_hit_light']}), light_edge_pairs {c64['light_edge_pairs']}; fragile rays {c64['rays_fragile']} of {c64['rays_launched']}")
    # the caps that keep the allowance from hiding a failure (proved on the tracer alone in the CPU file, held here at this spp)
    for k, (tested, blocked, edge) in enumerate(per_light):
        assert tested > 0 and edge <= EDGE_CAP * tested, (k, tested, edge)
        if k in partly:
            assert 0.1 < blocked / tested < 0.9, (k, blocked, tested)
    slack = c64["light_edge_pairs"] + o["edge"]
    _check_against_f64(img, cnt, ref, frag, c64, min_lit=min_lit, culled=culled, hit_light_slack=slack)
    # the device's tallies are the tracer's, up to the pairs either side calls undecidable
    assert abs(stats["tested"] - o["tested"]) <= c64["rays_fragile"] + c64["light_edge_pairs"], (stats, o)
    assert abs(stats["blocked"] - o["blocked"]) <= c64["rays_fragile"] + slack, (stats, o)
    assert 0 < stats["blocked"] < stats["tested"] and cnt["rays_hit_light"] == stats["tested"] - stats["blocked"]
    return img, cnt, stats, o


# ---- 1. the sky's reach ---------------------------------------------------------------------------------------------------------
def test_sun_behind_a_sphere_a_mesh_and_a_comb_within_1e4(pkg, lf, mask):
    """an analytic sphere, a tessellated one of 320 triangles (the device descends a tree, the tracer tests every triangle) and a
    comb of slats 2 mm in front of the first vertex, where hz and the ray's own direction decide"""
    _against_f64(pkg, lf, mask, "sun_sky", 256)


def test_two_suns_that_share_one_walk_within_1e4(pkg, lf, mask):
    """the branch without kVarNear walks once per lane and answers for both lights; the tracer decides each light on its own"""
    _, _, _, o = _against_f64(pkg, lf, mask, "two_suns_sky", 256)
    assert all(0 < b < t for t, b, _ in o["per_light"][:2])


# ---- 2. the light's reach -------------------------------------------------------------------------------------------------------
def test_a_lamp_behind_a_half_wall_and_in_front_of_a_full_one_within_1e4(pkg, lf, mask):
    _against_f64(pkg, lf, mask, "lamp_reach", 256)


def test_mixed_lights_behind_half_walls_at_three_depths_within_1e4(pkg, lf, mask):
    """[SUN, LAMP at 300 mm, LAMP2 at 90 mm, a tilted panel at 90 mm] under the light's reach: a lane's walks get reaches short after
    long and long after short (the interval reuse of lights_epilogue), and every light loses another share"""
    _, _, _, o = _against_f64(pkg, lf, mask, "mixed_reach", 256)
    assert all(0 < b < t for t, b, _ in o["per_light"][:4])
    shares = [b / t for t, b, _ in o["per_light"][:4]]
    assert max(shares) - min(shares) > 0.1, shares


@pytest.mark.parametrize("family,bits", [("culled", 6), ("items", 0)])
def test_mixed_lights_within_1e4_in_the_culled_march_and_the_item_kernel(pkg, lf, mask, forced, family, bits):
    _against_f64(pkg, lf, mask, "mixed_reach", 64, mode=2, bits=bits, label=f"mixed_reach, {family}", audit=True)


# ---- 3. one wavelength of three -------------------------------------------------------------------------------------------------
def test_last_wavelength_alone_starts_its_shadow_ray_where_its_own_ray_left_the_lens(pkg, lf, mask):
    _against_f64(pkg, lf, mask, "sun_sky_last_wavelength", 256)


# ---- 4. the pose ----------------------------------------------------------------------------------------------------------------
def test_an_occluder_that_moves_with_the_camera_is_the_same_occluder(pkg, lf, mask):
    """mixed_reach under the general pose and under the identity, the occluders carried along: the device frames are bit-identical
    (each is then the frame the tracer is compared with above)"""
    try:
        a, ca, sa, _ = _occluded_frame(pkg, lf, mask, "mixed_reach", 64, pose=POSE)
        b, cb, sb, _ = _occluded_frame(pkg, lf, mask, "mixed_reach", 64, pose=IDENTITY)
    finally:
        _restore(pkg, lf)
    assert a.max() > 0 and 0 < sa["blocked"] < sa["tested"]
    assert np.array_equal(a, b) and ca == cb and sa == sb
