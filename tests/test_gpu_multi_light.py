"""Several lights in ONE pass of the geometric march (lf_set_lights; lens-flare_amd/csrc: lights_pretest / lights_epilogue
in lf_march_common.h, the kVarLights kernels of lf_march.hip and lf_cull.hip, k_cull_resolve<true> / k_cull_level_lights /
k_cull_audit<true> in lf_cull_prepass.hip).  The reference keeps a flare list but one `angle_to_sun`
(src/pathtracer/pathtracer.cpp:45); its ghosts know one light.

Contributions are added as unsigned 64-bit fixed-point integers, one per (ray, light, channel), so the contract is sharp:
a frame of K lights is the SUM of the K single-light frames under the same key, sampling specification and `bits`, bit for
bit -- and the single-light frames are the float32 oracle's (oracle/lf_geo_oracle.c), which therefore checks every K-light
frame here without knowing about several lights.  spp is a power of two and `bits` 36 throughout (checked), so a frame
acc 2^-36 / spp and the sums of frames are exact in float64."""
import os
import subprocess

import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo

pytestmark = pytest.mark.gpu
RAD = [1.0, 0.9, 0.5]
RAD2 = [0.5, 1.0, 0.8]
MASK = "pentbig500_14.png"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "lens-flare_amd", "host", "shim_demo")
LF_ERR_INVALID, LF_ERR_STATE = 1, 4


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
    lfo.geo_follow_device(ctx)
    yield ctx
    lfo.geo_follow_device(None)
    ctx.close()


@pytest.fixture()
def forced(pkg, lf):
    """the culled march whatever the table starts (tests/test_gpu_cull.py): on the module's context and on every context
    created meanwhile"""
    lf.test_knob("cull_force", 1)
    pkg.test_knob_default("cull_force", 1)
    yield
    lf.test_knob("cull_force", 0)
    pkg.test_knob_default("cull_force", 0)


def _crop(lens, W, pitch_of=1920):
    """the prescription on a sensor W pixels wide at the pixel pitch of a 36 mm sensor `pitch_of` pixels wide"""
    c = dict(lens)
    c["sensor_width_mm"] = 36.0 * W / pitch_of
    return c


def _setup(pkg, lf, lens, W, H, mask, lambda_rgb=None):
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    if lambda_rgb is not None:
        lf.set_lambda_rgb(lambda_rgb)
    lf.set_ghost_pairs(None, True)
    lf.set_band(0, H)
    lf.set_row_interleave(0, 1)
    lf.set_tile_stride(8)
    lf.set_pupil_subcells(6)
    lf.set_mask_filter(pkg.MASK_NEAREST)
    lf.set_ghost_accumulate(False)


def _install(lf, lights):
    """lights: [(direction, radiance, angular radius), ...]"""
    lf.set_lights([l[0] for l in lights], [l[1] for l in lights], [l[2] for l in lights])


def _frame(pkg, lf, spp, key, mode):
    lf.set_march_culling(mode)
    lf.reset_counters()
    lf.trace_ghosts(spp, key)
    assert lf.march_fix_bits() == 36
    return lf.read_buffer(pkg.GHOST_BUFFER), lf.counters()


def _oracle(lens, W, H, spp, key, mask, lights, lambda_rgb=None):
    """the float32 oracle's full enumeration, one light at a time -> [(frame, counters)]"""
    return [lfo.geo_trace(lens, W, H, 0, H, spp, key, None, True, mask, d, r, a, n_threads=16, lambda_rgb=lambda_rgb, cull=None)
            for d, r, a in lights]


# the second lobe overlaps the first (some rays lie in both); the third is small and has another radiance
THREE = [([0.03, 0.02, -1.0], RAD, 0.05), ([0.035, 0.02, -1.0], RAD, 0.05), ([-0.06, 0.04, -1.0], RAD2, 0.004)]


def test_sum_of_single_light_frames_is_the_oracle_uncut(pkg, lf, mask):
    W, H, spp, key = 48, 32, 16, 0x11A7
    lens = pkg.load_lens_file("dgauss11.lens")
    _setup(pkg, lf, lens, W, H, mask)
    _install(lf, THREE)
    g, c = _frame(pkg, lf, spp, key, 0)
    assert not lf.cull_info()["culled"]
    o = _oracle(lens, W, H, spp, key, mask, THREE)
    want = o[0][0] + o[1][0] + o[2][0]
    assert np.array_equal(g, want) and want.max() > 0
    # the overlap is real: some pixel is lit by both of the overlapping lights, and the small lobe lights something too
    assert ((o[0][0] > 0) & (o[1][0] > 0)).any() and o[2][0].max() > 0
    # the rays, their events and their fates know no light; rays_hit_light counts (ray, light) contributions
    for name, v in c.items():
        if name == "rays_hit_light":
            assert v == sum(oc[name] for _, oc in o) and v > 0
        else:
            assert all(v == oc[name] for _, oc in o), name


def test_the_same_light_twice_and_one_light_through_set_lights(pkg, lf, mask):
    W, H, spp, key = 48, 32, 16, 0x11A8
    lens = pkg.load_lens_file("dgauss11.lens")
    _setup(pkg, lf, lens, W, H, mask)
    d, r, a = THREE[0]
    lf.set_sun(d, r, a)
    g1, c1 = _frame(pkg, lf, spp, key, 0)
    sun_state = lf.lights()
    _install(lf, [THREE[0]])
    g1l, c1l = _frame(pkg, lf, spp, key, 0)
    assert np.array_equal(g1, g1l) and c1 == c1l and g1.max() > 0
    assert all(np.array_equal(x, y) for x, y in zip(sun_state, lf.lights()))
    _install(lf, [THREE[0], THREE[0]])
    g2, c2 = _frame(pkg, lf, spp, key, 0)
    assert np.array_equal(g2, 2.0 * g1)
    assert c2["rays_hit_light"] == 2 * c1["rays_hit_light"]
    assert {k: v for k, v in c2.items() if k != "rays_hit_light"} == {k: v for k, v in c1.items() if k != "rays_hit_light"}


def _table_of(lf, spp, key, lights, cache=True):
    """the table of one launch that marches one tile row only (the pre-pass does not depend on the band)"""
    _install(lf, lights)
    lf.set_march_culling(2)
    lf.test_knob("cull_cache", 1 if cache else 0)
    try:
        lf.trace_ghosts(spp, key)
    finally:
        lf.test_knob("cull_cache", 1)
    assert lf.cull_info()["culled"], lf.cull_reason()
    return lf.cull_table()


# (130 x 70: three blocks across; the lights' images fall in different blocks, the third light lies outside the frame's field)
@pytest.mark.parametrize("W,H,spp,lights", [
    (96, 64, 64, [([0.012, 0.004, -1.0], RAD, 0.02), ([-0.010, -0.006, -1.0], RAD2, 0.05)]),
    (130, 70, 16, [([0.02, 0.003, -1.0], RAD, 0.02), ([-0.02, -0.004, -1.0], RAD2, 0.03), ([0.15, 0.05, -1.0], RAD, 0.05)])])
def test_culled_is_the_full_enumeration_and_the_table_is_the_or(pkg, mask, forced, W, H, spp, lights):
    key = 0xC011 + spp
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    ctx = pkg.LensFlare(0)        # (a context of its own: the cache's policy remembers what a context was asked before)
    try:
        ctx.timing_enable(True)
        _setup(pkg, ctx, lens, W, H, mask)
        _install(ctx, lights)
        g2, c2 = _frame(pkg, ctx, spp, key, 2)
        assert ctx.cull_info()["culled"] and ctx.cull_reason() == "applied", ctx.cull_reason()
        audit = ctx.cull_audit()
        assert audit["rays"] > 0 and audit["lit"] == 0 and audit["launches_refuted"] == 0
        table = ctx.cull_table()
        builds = ctx.timing_get("cull_cache_build")[0]
        assert builds >= 1
        g0, c0 = _frame(pkg, ctx, spp, key, 0)
        assert not ctx.cull_info()["culled"]
        assert np.array_equal(g2, g0) and c2["rays_hit_light"] == c0["rays_hit_light"] > 0
        assert 0 < c2["rays_launched"] < c0["rays_launched"]
        want = sum(f for f, _ in _oracle(lens, W, H, spp, key, mask, lights))
        assert np.array_equal(g0, want) and want.max() > 0
        # the K-light table is the bitwise OR of the K single-light tables (the cached resolve) ...
        ctx.set_band(0, 8)
        singles = [_table_of(ctx, spp, key, [l]) for l in lights]
        union = singles[0].copy()
        for t in singles[1:]:
            union |= t
        assert np.array_equal(table, union)
        assert any(not np.array_equal(t, union) for t in singles)        # (no light's table is the whole of it)
        # ... and a superset of it without the cached tree (a box is kept unless every light's lobe rules it out), same frame
        uncached = _table_of(ctx, spp, key, lights, cache=False)
        assert not (union & ~uncached).any()
        ctx.set_band(0, H)
        ctx.test_knob("cull_cache", 0)
        try:
            gu, _ = _frame(pkg, ctx, spp, key, 2)
        finally:
            ctx.test_knob("cull_cache", 1)
        assert ctx.cull_info()["culled"] and np.array_equal(gu, g0)
        # any light decides the table: moving one changes it, the old lights bring it back -- and the tree is not built again
        ctx.set_band(0, 8)
        moved = list(lights)
        moved[-1] = ([-lights[-1][0][0], lights[-1][0][1] + 0.01, -1.0], lights[-1][1], lights[-1][2])
        assert not np.array_equal(_table_of(ctx, spp, key, moved), table)
        assert np.array_equal(_table_of(ctx, spp, key, lights), table)
        assert ctx.timing_get("cull_cache_build")[0] == builds
    finally:
        ctx.close()


TWO = [([0.012, 0.004, -1.0], RAD, 0.03), ([-0.014, -0.006, -1.0], RAD2, 0.05)]


def test_every_kernel_family(pkg, lf, mask, forced):
    W, H, spp, key = 80, 48, 64, 0xFA31
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    _install(lf, TWO)
    g0, c0 = _frame(pkg, lf, spp, key, 0)
    assert g0.max() > 0
    try:
        for stride, bits in [(8, 6), (8, 0)]:      # (8, 0): independent pixels, the compacted march (k_march_items)
            lf.set_tile_stride(stride)
            lf.set_pupil_subcells(bits)
            full, cf = _frame(pkg, lf, spp, key, 0)
            g, c = _frame(pkg, lf, spp, key, 2)
            assert lf.cull_info()["culled"]
            assert np.array_equal(g, full) and c["rays_hit_light"] == cf["rays_hit_light"] > 0, (stride, bits)
            if bits == 6:
                assert np.array_equal(full, g0)
        lf.set_pupil_subcells(6)
        for knob in ("cull_no_prefix", "cull_weights_first"):      # every started path alone / the weight on every event
            lf.test_knob(knob, 1)
            try:
                g, c = _frame(pkg, lf, spp, key, 2)
            finally:
                lf.test_knob(knob, 0)
            assert lf.cull_info()["culled"]
            assert np.array_equal(g, g0) and c["rays_hit_light"] == c0["rays_hit_light"], knob
    finally:
        lf.set_tile_stride(8)
        lf.set_pupil_subcells(6)


def test_eight_wavelengths(pkg, lf, mask, forced):
    W, H, spp, key = 32, 24, 16, 0x8A3B
    lens = _crop(pkg.load_lens_file("dgauss11_8lambda.lens"), W)
    lam = pkg.spectral_weights(lens["lambda_nm"])[0]
    _setup(pkg, lf, lens, W, H, mask, lam)
    _install(lf, TWO)
    g2, _ = _frame(pkg, lf, spp, key, 2)
    assert lf.cull_info()["culled"]
    g0, _ = _frame(pkg, lf, spp, key, 0)
    want = sum(f for f, _ in _oracle(lens, W, H, spp, key, mask, TWO, lam))
    assert np.array_equal(g2, g0) and np.array_equal(g0, want) and want.max() > 0


@pytest.mark.parametrize("variant", ["coated", "bilinear"])
def test_films_and_the_bilinear_mask_combine_with_several_lights(pkg, lf, mask, forced, variant):
    """(the float32 oracle follows neither feature: the frame is held against the device's own single-light frames of the
    same variant, which tests/test_gpu_coatings.py and tests/test_gpu_mask_filter.py pin)"""
    W, H, spp, key = 64, 48, 64, 0x7A21
    lens = _crop(pkg.load_lens_file("dgauss11_coated.lens" if variant == "coated" else "dgauss11.lens"), W)
    _setup(pkg, lf, lens, W, H, mask)
    if variant == "bilinear":
        lf.set_mask_filter(pkg.MASK_BILINEAR)
    try:
        _install(lf, TWO)
        g2, c2 = _frame(pkg, lf, spp, key, 2)
        assert lf.cull_info()["culled"]
        g0, c0 = _frame(pkg, lf, spp, key, 0)
        assert np.array_equal(g2, g0) and c2["rays_hit_light"] == c0["rays_hit_light"] > 0
        singles = []
        for l in TWO:
            _install(lf, [l])
            singles.append(_frame(pkg, lf, spp, key, 0)[0])
        assert np.array_equal(g0, singles[0] + singles[1]) and singles[0].max() > 0 and singles[1].max() > 0
    finally:
        lf.set_mask_filter(pkg.MASK_NEAREST)
        lf.set_lens_coatings(None)


def _geom_norm(lens):
    """LfLensDev::geom_norm as lf_derive_lens / lf_apply_pupil_target compute it"""
    z = np.float32(0.0)
    zs = []
    for t in np.asarray(lens["thickness"], np.float32):
        zs.append(z)
        z = np.float32(z + t)
    h = float(np.float32(lens["semi_aperture"][-1]))
    D = float(z) - float(zs[-1])
    return float(np.float32(np.pi * h * h / (D * D)))


def test_max_lights_and_the_range_contract(pkg, lf, mask):
    W, H, spp, key = 32, 24, 16, 0x8888
    lens = pkg.load_lens_file("dgauss11.lens")
    _setup(pkg, lf, lens, W, H, mask)
    n = pkg.MAX_LIGHTS
    ring = [([0.04 * np.cos(2 * np.pi * k / n), 0.04 * np.sin(2 * np.pi * k / n), -1.0], [0.25 + 0.125 * (k % 3), 0.5, 0.125 * (1 + k % 4)], 0.05)
            for k in range(n)]
    _install(lf, ring)
    g, c = _frame(pkg, lf, spp, key, 0)
    o = _oracle(lens, W, H, spp, key, mask, ring)
    assert np.array_equal(g, sum(f for f, _ in o)) and g.max() > 0
    assert c["rays_hit_light"] == sum(oc["rays_hit_light"] for _, oc in o)
    # HDR: the launch leaves the default grid; the exponent is lf_march_fix_bits' rule for the SUMMED radiance
    hdr = [(d, [float(np.float32(v) * 2.0 ** 30) for v in r], a) for d, r, a in ring]
    _install(lf, hdr)
    lf.set_march_culling(0)
    lf.trace_ghosts(spp, key)
    worst = max(sum(float(np.float32(r[ch])) for _, r, _ in hdr) for ch in range(3))      # (lambda_rgb: the identity)
    worst *= spp * 46 * _geom_norm(lens)
    bits = 36
    while worst * 2.0 ** bits >= 2.0 ** 62:
        bits -= 1
    assert bits < 36 and lf.march_fix_bits() == bits
    g1 = lf.read_buffer(pkg.GHOST_BUFFER)
    _install(lf, [(d, [2.0 * v for v in r], a) for d, r, a in hdr])
    lf.trace_ghosts(spp, key)
    assert lf.march_fix_bits() == bits - 1
    assert np.array_equal(lf.read_buffer(pkg.GHOST_BUFFER), 2.0 * g1) and g1.max() > 0


def test_the_audit_sees_every_light(pkg, mask, forced):
    """a table built WITHOUT light 1 (lf_test_knob cull_ignore_light) drops boxes whose rays end inside light 1's lobe: the
    audit, which marches with every light, refutes it and the launch falls back to the full enumeration"""
    W, H, spp, key = 96, 64, 64, 0xA0D1
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    lights = [([0.014, 0.0, -1.0], RAD, 0.02), ([-0.014, 0.0, -1.0], RAD2, 0.02)]      # their images: different halves of the frame
    ctx = pkg.LensFlare(0)
    try:
        _setup(pkg, ctx, lens, W, H, mask)
        _install(ctx, lights)
        g0, c0 = _frame(pkg, ctx, spp, key, 0)
        ctx.test_knob("cull_ignore_light", 1)
        g, c = _frame(pkg, ctx, spp, key, 2)
        audit = ctx.cull_audit()
        assert audit["launches_refuted"] >= 1 and audit["lit"] > 0
        assert ctx.cull_reason() == "audit_refuted" and not ctx.cull_info()["culled"]
        assert np.array_equal(g, g0) and c == c0 and g0.max() > 0
        ctx.test_knob("cull_ignore_light", -1)
        g, c = _frame(pkg, ctx, spp, key, 2)
        audit = ctx.cull_audit()
        assert audit["launches_refuted"] == 0 and audit["lit"] == 0 and audit["rays"] > 0
        assert ctx.cull_reason() == "applied" and ctx.cull_info()["culled"]
        assert np.array_equal(g, g0) and c["rays_hit_light"] == c0["rays_hit_light"]
    finally:
        ctx.close()


def test_refusals_and_lifecycle(pkg, mask):
    W, H = 32, 24
    lens = pkg.load_lens_file("dgauss11.lens")
    ctx = pkg.LensFlare(0)
    try:
        _setup(pkg, ctx, lens, W, H, mask)
        assert len(ctx.lights()[0]) == 0
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.trace_ghosts(4, 1)
        assert e.value.status == LF_ERR_STATE
        _install(ctx, THREE)
        d, r, a = ctx.lights()
        assert len(d) == 3 and np.array_equal(r, np.array([l[1] for l in THREE], np.float32))
        assert np.array_equal(a, np.array([l[2] for l in THREE], np.float32))
        for k, l in enumerate(THREE):
            v = np.asarray(l[0], np.float32).astype(np.float64)      # (normalised in double from the floats handed over, then narrowed)
            assert np.array_equal(d[k], (v / np.sqrt((v * v).sum())).astype(np.float32))
        good = ([0.0, 0.0, -1.0], RAD, 0.05)
        nine = [good] * (pkg.MAX_LIGHTS + 1)
        bad = [[], nine,
               [good, ([float("nan"), 0.0, -1.0], RAD, 0.05)], [good, ([0.1, 0.0, 0.0], RAD, 0.05)], [good, ([0.1, 0.0, 0.5], RAD, 0.05)],
               [good, ([0.0, 0.0, -1.0], [1.0, -0.5, 1.0], 0.05)], [good, ([0.0, 0.0, -1.0], RAD, 0.0)], [good, ([0.0, 0.0, -1.0], RAD, 1.6)]]
        for lights in bad:
            with pytest.raises(pkg.LensFlareError) as e:
                _install(ctx, lights)
            assert e.value.status == LF_ERR_INVALID, lights
            now = ctx.lights()
            assert all(np.array_equal(x, y) for x, y in zip(now, (d, r, a)))          # the previous lights stay
        # lf_set_lens / lf_set_frame keep the lights, as they keep the sun
        ctx.set_lens(lens)
        ctx.set_frame(W + 8, H)
        ctx.set_aperture(pkg.APERTURE_STARBURST, mask)
        assert all(np.array_equal(x, y) for x, y in zip(ctx.lights(), (d, r, a)))
        ctx.trace_ghosts(4, 1)
        assert ctx.read_buffer(pkg.GHOST_BUFFER).max() > 0
    finally:
        ctx.close()


def _lens_txt(lens, path):
    n, nl = lens["n"], lens["ior"].shape[0]
    with open(path, "w") as f:
        f.write(f"{n} {lens['stop']} {nl} {lens['sensor_width_mm']!r}\n")
        for k in range(n):
            row = [lens["radius"][k], lens["thickness"][k], lens["semi_aperture"][k]] + [lens["ior"][l, k] for l in range(nl)]
            f.write(" ".join(repr(float(v)) for v in row) + "\n")


def test_hand_over_from_the_flare_state(pkg, mask, tmp_path):
    W, H, spp, key = 48, 32, 16, 0x1e45f1a4e
    lens = pkg.load_lens_file("dgauss11.lens")
    ctx = pkg.LensFlare(0)
    try:
        _setup(pkg, ctx, lens, W, H, mask)
        ctx.set_camera(np.eye(3).reshape(-1), [0.0, 0.0, 0.0], 40.0, 27.0)
        inside = [[0.5, 0.3, -10.0] + RAD, [-1.2, -0.4, -10.0] + RAD2]
        ctx.find_sun_pos(inside + [[30.0, 0.0, -10.0] + RAD])              # the third is out of the frame
        assert ctx.set_lights_from_flares(0.0, 0.05) == 2
        got = ctx.lights()
        g2, c2 = _frame(pkg, ctx, spp, key, 0)
        singles = []
        for k in range(2):
            ctx.set_sun_from_flares(k, 0.0, 0.05)
            one = ctx.lights()
            assert all(np.array_equal(x[k], y[0]) for x, y in zip(got, one))
            singles.append(_frame(pkg, ctx, spp, key, 0))
        assert np.array_equal(g2, singles[0][0] + singles[1][0]) and min(s[0].max() for s in singles) > 0
        assert c2["rays_hit_light"] == singles[0][1]["rays_hit_light"] + singles[1][1]["rays_hit_light"]
        # one in-frame light: the installed state and the frame are lf_set_sun_from_flares(0)'s
        ctx.find_sun_pos(inside[:1])
        ctx.set_sun_from_flares(0, 0.0, 0.05)
        want_state, want = ctx.lights(), _frame(pkg, ctx, spp, key, 0)
        _install(ctx, THREE)
        assert ctx.set_lights_from_flares(0.0, 0.05) == 1
        assert all(np.array_equal(x, y) for x, y in zip(ctx.lights(), want_state))
        g, c = _frame(pkg, ctx, spp, key, 0)
        assert np.array_equal(g, want[0]) and c == want[1]
        # more in-frame lights than one launch follows: refused, the limit named, the lights untouched
        ctx.find_sun_pos([[0.2 * k - 0.8, 0.1, -10.0] + RAD for k in range(pkg.MAX_LIGHTS + 1)])
        with pytest.raises(pkg.LensFlareError) as e:
            ctx.set_lights_from_flares(0.0, 0.05)
        assert e.value.status == LF_ERR_INVALID and "LF_MAX_LIGHTS = %d" % pkg.MAX_LIGHTS in str(e.value)
        assert all(np.array_equal(x, y) for x, y in zip(ctx.lights(), want_state))
        # ---- one frame through the host mirror's frame sequence (lf_frame_sequence.h) with two in-frame lights
        assert os.path.exists(DEMO), "run __graft_entry__.build() first"
        origins, radiance = [[0.62, 0.55], [0.3, 0.4]], [RAD, RAD2]
        _lens_txt(lens, tmp_path / "lens.txt")
        mask.tofile(tmp_path / "mask.f32")
        out = str(tmp_path / "m")
        args = [DEMO, "geolights", str(tmp_path / "lens.txt"), str(tmp_path / "mask.f32"), str(mask.shape[1]), str(mask.shape[0]),
                str(W), str(H), str(spp), "0.05", out, "2"]
        for o, r in zip(origins, radiance):
            args += [repr(float(v)) for v in o + r]
        run = subprocess.run(args, capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        ghost = np.fromfile(out + ".ghost.f64", np.float64).reshape(H, W, 3)
        ctx.set_flares(origins, radiance, [0.5, 0.5], 0.0)
        parts = []
        for k in range(2):
            ctx.set_sun_from_flares(k, 0.0, 0.05)
            parts.append(_frame(pkg, ctx, spp, key, 0)[0])
        assert np.array_equal(ghost, parts[0] + parts[1]) and parts[0].max() > 0 and parts[1].max() > 0
    finally:
        ctx.close()


def test_two_contexts_under_the_block_deal(pkg, mask, forced):
    W, H, spp, key = 130, 70, 16, 0xB10C
    lens = _crop(pkg.load_lens_file("dgauss11.lens"), W)
    lights = [([0.02, 0.003, -1.0], RAD, 0.02), ([-0.02, -0.004, -1.0], RAD2, 0.03)]

    def render(rank, n):
        ctx = pkg.LensFlare(0)
        try:
            _setup(pkg, ctx, lens, W, H, mask)
            _install(ctx, lights)
            if n > 1:
                ctx.set_block_deal(rank, n)
            g, c = _frame(pkg, ctx, spp, key, 2)
            assert ctx.cull_info()["culled"], ctx.cull_reason()
            assert ctx.cull_audit()["lit"] == 0
            return g, c
        finally:
            ctx.close()

    want, wc = render(0, 1)
    bx = (W + 63) // 64
    yy, xx = np.mgrid[0:H, 0:W]
    owner = ((yy // 64) * bx + xx // 64) % 2
    got, hits = np.zeros_like(want), 0
    for r in range(2):
        g, c = render(r, 2)
        got[owner == r] = g[owner == r]
        hits += c["rays_hit_light"]
    assert np.array_equal(got, want) and want.max() > 0 and hits == wc["rays_hit_light"]
