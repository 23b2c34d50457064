"""Aspheric interfaces on the device (lf_set_lens_aspheres; lens-flare_amd/csrc/lf_asphere.h, lf_march_asph.hip): the event's
host and device twins bit for bit, lf_march_path_rays against the kernels and the oracle that exist, k_march_asph against the
float64 tracer through "asph_force", the aspheric lens against tests/asphere_ref.py, the frame identities, the routing, and --
they need a context -- the setter, the getter and the C parser."""
import os

import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo

import asphere_ref as ar
from test_area_ghosts_cpu import RECTS, AREA, geom_of
from test_aspheres_cpu import _surfaces, _yardstick, _rays, COS_MIN
from test_gpu_march_f64 import _check_against_f64, TOL, FLOOR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = "pentbig500_14.png"
W, H, SPP, KEY = 128, 64, 16, 0xA5F
SUN = (0, [0.012, 0.004, -1.0], [0.5, 1.0, 0.125], 0.03)
LAMP = (1, [1.5, -1.0, -90.0], [0.25, 0.125, 1.0], 0.05)
PANEL = (AREA, geom_of(RECTS[0]), [1.0, 0.5, 0.25], 0.0)
LF_ERR_INVALID, LF_ERR_UNSUPPORTED = 1, 6


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
def asph(pkg):
    return pkg.load_lens_file("dgauss11_asph.lens")


@pytest.fixture(scope="module")
def plain(pkg):
    return pkg.load_lens_file("dgauss11.lens")


def _setup(pkg, ctx, lens, mask, lights=(SUN,)):
    ctx.set_frame(W, H)
    ctx.set_aperture(pkg.APERTURE_STARBURST, mask)
    ctx.set_lens(lens)
    ctx.set_ghost_pairs(None, True)
    ctx.set_band(0, H)
    ctx.set_row_interleave(0, 1)
    ctx.set_mask_filter(pkg.MASK_NEAREST)
    ctx.set_ghost_accumulate(False)
    ctx.set_ghost_occlusion(False)
    ctx.set_march_culling(1)
    ctx.set_lights_geom([l[0] for l in lights], [l[1] for l in lights], [l[2] for l in lights], [l[3] for l in lights])


def _frame(pkg, ctx, spp=SPP, key=KEY):
    ctx.reset_counters()
    ctx.trace_ghosts(spp, key)
    return ctx.read_buffer(pkg.GHOST_BUFFER).copy(), ctx.counters()


# ---- the event: host against device ---------------------------------------------------------------------------------------
def test_the_device_event_is_the_host_event_bit_for_bit(pkg, lf):
    lf.set_frame(W, H)
    for s in _surfaces():
        for forward in (0, 1):
            for reflect in (0, 1):
                p, d, z0 = _rays(s["h"], forward, 200 + 2 * forward + reflect)
                p, d = p[:1024], d[:1024]
                n_in, n_out = (s["n_before"], s["n_after"]) if forward else (s["n_after"], s["n_before"])
                rays = np.concatenate([p[:, :2], np.zeros((len(p), 1), np.float32), d * np.float32(n_in)], axis=1).astype(np.float32)
                args = (s["c"], s["kappa"], s["A"], s["h"], n_in, n_out, reflect, forward, z0, rays)
                ho, hf = pkg.asphere_event(*args)
                do, df = lf.asphere_events(*args)
                assert np.array_equal(hf, df)
                assert len(np.unique(hf)) >= 2                      # (the rays meet more than one fate)
                # every field of a ray that lives, bit for bit, and none of them a NaN ...
                live = hf == 0
                assert not np.isnan(ho[live]).any() and not np.isnan(do[live]).any()
                assert np.array_equal(ho[live].view(np.uint32), do[live].view(np.uint32))
                # ... and of a dead ray too, but for the bits of a NaN: a NaN on both sides (its sign is the processor's)
                assert np.array_equal(np.isnan(ho), np.isnan(do))
                num = ~np.isnan(ho)
                assert np.array_equal(ho.view(np.uint32)[num], do.view(np.uint32)[num])


# ---- the instrument -------------------------------------------------------------------------------------------------------
def test_path_rays_are_the_kernels_and_the_oracle_that_exist(pkg, lf, plain, mask):
    _setup(pkg, lf, plain, mask)
    xy, uv = ar.comparison_grid()
    for lam in (0, 2):
        a = lf.march_path_rays(lam, -1, -1, xy, uv)
        b = lf.generate_lens_rays(lam, xy, uv)
        assert a[:, 7].sum() > 100 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # ghost pairs: sensor points on the y axis, pupil points on the x axis -- there the start ray needs no polynomial:
    # v = (h pa, -Y, vz), d = v rcp(sqrt(|v|^2)) with the device's own root and reciprocal
    n = 1365
    rng = np.random.default_rng(5)
    Y = rng.uniform(-10, 10, n).astype(np.float32); pa = rng.uniform(-0.95, 0.95, n).astype(np.float32)
    pa[pa == 0] = 0.5
    xy = np.stack([np.zeros(n, np.float32), Y], axis=1); uv = np.stack([pa, np.zeros(n, np.float32)], axis=1)
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    hp = np.float32(plain["semi_aperture"][-1])
    zs = np.float32(lfo.geo_z_sensor(plain))
    pz = np.cumsum(np.asarray(plain["thickness"][:-1], np.float32), dtype=np.float32)[-1]     # the rear vertex, summed as floats
    vz = np.float32(pz - zs)
    lfo.geo_follow_device(lf)
    try:
        vx = (hp * pa).astype(np.float32); vy = (-Y).astype(np.float32)
        inner = (f64(vy) * f64(vy) + f64(np.float32(vz * vz))).astype(np.float32)          # fmaf(vy, vy, vz * vz)
        ss = (f64(vx) * f64(vx) + f64(inner)).astype(np.float32)                             # fmaf(vx, vx, .)
        rl = lf.native_rcp(lf.native_sqrt(ss))
        d = np.stack([vx * rl, vy * rl, np.full(n, vz, np.float32) * rl], axis=1).astype(np.float32)
        gn = np.float32((np.pi * float(hp) * float(hp)) / ((float(zs) - float(pz)) ** 2))
        for (i, j) in ((0, 1), (2, 8), (6, 10)):
            got = lf.march_path_rays(1, i, j, xy, uv)
            same = 0
            for k in range(0, n, 7):
                c2 = d[k, 2] * d[k, 2]
                w0 = np.float32(gn * np.float32(c2 * c2))
                st, pe, de, w, ne = lfo.geo_trace_ray(plain, 1, i, j, [0.0, Y[k], zs], d[k], float(w0), mask)
                assert (st == 0) == (got[k, 7] == 1.0), (i, j, k, st, got[k])
                if st == 0:
                    want = np.array([pe[0], pe[1], pe[2], de[0], de[1], de[2], w], np.float32)
                    assert np.array_equal(want.view(np.uint32), got[k, :7].view(np.uint32)), (i, j, k, want, got[k])
                    same += 1
            assert same >= 20, (i, j, same)
    finally:
        lfo.geo_follow_device(None)


# ---- the kernel against the float64 oracle that exists --------------------------------------------------------------------
def test_the_aspheric_kernel_passes_the_path_trees_float64_comparison(pkg, lf, plain, mask):
    """"asph_force" on dgauss11.lens under LF_MASK_BILINEAR: every curved glass row takes the Newton path with a zero record.
    The helper and the bar are tests/test_gpu_march_f64.py's; the frame needs the fragile-ray allowance for no more values
    than the path tree's own frame of the same inputs."""
    sun, rad, alpha = [0.03, 0.02, -1.0], [1.0, 0.9, 0.5], 0.05
    need = {}
    lfo.g64_set_mask_filter(1)
    try:
        ref, frag, c64 = lfo.g64_trace(plain, W, H, 0, H, SPP, KEY, None, True, mask, sun, rad, alpha, n_threads=16, cull=None)
        for name, force in (("tree", 0), ("asph", 1)):
            _setup(pkg, lf, plain, mask)
            lf.set_mask_filter(pkg.MASK_BILINEAR)
            lf.set_march_culling(0)
            lf.set_sun(sun, rad, alpha)
            lf.test_knob("asph_force", force)
            img, cnt = _frame(pkg, lf)
            assert (lf.cull_reason() == "aspheric") == bool(force)
            _check_against_f64(img, cnt, ref, frag, c64, min_lit=100)
            lit = ref >= FLOOR
            need[name] = int((np.abs(img - ref)[lit] > TOL * ref[lit]).sum())
    finally:
        lf.test_knob("asph_force", 0)
        lfo.g64_set_mask_filter(0)
        lf.set_mask_filter(pkg.MASK_NEAREST)
        lf.set_march_culling(1)
    print("values on the fragile-ray allowance:", need)
    assert need["asph"] <= need["tree"], need


# ---- real aspheres --------------------------------------------------------------------------------------------------------
def _pairs(lens):
    g = [k for k in range(lens["n"]) if k != lens["stop"]]
    return [(-1, -1)] + [(i, j) for a, i in enumerate(g) for j in g[a + 1:]]


@pytest.fixture(scope="module")
def traced(pkg, asph, plain, mask):
    """the float64 tracer over the fixed grid, once for both cases below: the primary path and every pair of dgauss11.lens
    (the weight's yardstick) and of the aspheric lens, each with dgauss11_coated.lens's films and bare"""
    xy, uv = ar.comparison_grid()
    coat = pkg.load_lens_file("dgauss11_coated.lens")["coatings"]
    out = dict(xy=xy, uv=uv, coat=coat, base={}, paths={})
    for (i, j) in _pairs(asph):
        out["base"][(i, j)] = ar.trace_path(plain, 1, i, j, xy, uv, mask, coat)
        out["paths"][(i, j)] = ar.trace_path(asph, 1, i, j, xy, uv, mask, coat)
    return out


@pytest.mark.parametrize("films", [False, True])
def test_the_aspheric_lens_against_the_float64_tracer(pkg, lf, asph, plain, mask, traced, films):
    """primary path and every pair over a fixed grid: exit point, direction, weight and alive / dead.  The bar ACCUMULATES the
    event's 4 D linearly over the path's events: an event may add 4 D to what the ray carries in position (mm) and in a
    direction component, so after e events the bar is 4 D e for both.  The WEIGHT has a yardstick of its own, taken like D
    from code that exists: Dw is the largest relative deviation, from the same tracer over the same grid, of the weights
    the spherical march gives on dgauss11.lens (lf_march_path_rays there runs the existing events, bit for bit the
    oracle's: the test above) -- for the primary path and for the ghost pairs separately, a ghost's weight holding two
    reflectances, small differences of float32 terms; the bar is 4 Dw.  Dw is itself held down: on every path of the
    spherical lens the march's weight stays within the relative 4 D n_ev that the path's position and direction get, so
    a bad yardstick fails here and widens nothing.  Rays the tracer finds within the bar of an
    aperture rim or at incidence cosine below 0.05 are left out: at most 2 % of the grid (tests/test_aspheres_cpu.py
    checks the tracer's side of that cap).  films: the same comparison with dgauss11_coated.lens's films on the lens."""
    D = max(_yardstick(s) for s in _surfaces())
    xy, uv, coat = traced["xy"], traced["uv"], traced["coat"]
    weight = (lambda t: t[0][:, 6]) if films else (lambda t: t[4])
    base = dict(plain)
    if films:
        base["coatings"] = coat
    _setup(pkg, lf, base, mask)
    Dw = {True: 0.0, False: 0.0}                       # [is the primary path]
    Dw_over = 0.0                                      # the yardstick's own limit: see below
    for (i, j), t in traced["base"].items():
        ex = lf.march_path_rays(1, i, j, xy, uv)
        n_ev = len(ar.sequence(plain["n"], i, j))
        ok0 = (ex[:, 7] == 1) & (t[0][:, 7] == 1) & (t[1] > COS_MIN) & (t[2] > 4 * D * n_ev)
        if ok0.any():
            w0 = weight(t)
            dev0 = float(np.max(np.abs(ex[ok0, 6] - w0[ok0]) / w0[ok0]))
            Dw[i < 0] = max(Dw[i < 0], dev0)
            Dw_over = max(Dw_over, dev0 / (4 * D * n_ev))
    # Dw may not widen the bar at will: on no path does the spherical march's weight deviate by more, relatively, than the
    # accumulated 4 D n_ev that position and direction get
    print(f"films {films}: Dw = {Dw[True]:.3e} (primary) / {Dw[False]:.3e} (ghosts), at most {Dw_over:.3f} of 4 D n_ev on any path")
    assert Dw_over <= 1.0, Dw_over
    lens = dict(asph)
    if films:
        lens["coatings"] = coat
    _setup(pkg, lf, lens, mask)
    G = ar.lens_geometry(lens)
    left_out = total = 0
    worst = dict(pos=0.0, dir=0.0, w=0.0)
    for (i, j) in _pairs(lens):
        got = lf.march_path_rays(1, i, j, xy, uv)
        t = traced["paths"][(i, j)]
        ref, cmin, rim, wref = t[0], t[1], t[2], weight(t)
        n_ev = len(ar.sequence(G["n"], i, j))
        bar_dir = bar_pos = 4 * D * n_ev
        bar_w = 4 * Dw[i < 0]
        skip = (rim <= bar_pos) | (cmin <= COS_MIN)
        left_out += int(skip.sum()); total += len(xy)
        keep = ~skip
        assert np.array_equal(got[keep, 7] == 1, ref[keep, 7] == 1), (i, j)
        a = keep & (ref[:, 7] == 1)
        if a.any():
            worst["pos"] = max(worst["pos"], float(np.max(np.abs(got[a, 0:3] - ref[a, 0:3])) / bar_pos))
            worst["dir"] = max(worst["dir"], float(np.max(np.abs(got[a, 3:6] - ref[a, 3:6])) / bar_dir))
            worst["w"] = max(worst["w"], float(np.max(np.abs(got[a, 6] - wref[a]) / wref[a]) / bar_w))
    print(f"films {films}: D = {D:.3e}, Dw = {Dw[True]:.3e} (primary) / {Dw[False]:.3e} (ghosts); worst deviation / bar: {worst}; left out {left_out} of {total}")
    assert left_out <= 0.02 * total
    assert worst["pos"] <= 1.0 and worst["dir"] <= 1.0 and worst["w"] <= 1.0, worst


# ---- frame identities on the aspheric lens (all bit for bit) --------------------------------------------------------------
def test_the_frame_is_the_sum_of_its_pairs_and_of_its_lights(pkg, lf, asph, mask):
    lights = [SUN, LAMP, PANEL]
    _setup(pkg, lf, asph, mask, lights)
    whole, cnt = _frame(pkg, lf)
    assert lf.cull_reason() == "aspheric" and whole.max() > 0
    fix = lf.march_fix_bits()
    # ... of per-pair launches under lf_set_ghost_accumulate (integer sums over 16 samples: every addition is exact)
    pairs = _pairs(asph)[1:]
    for n, (i, j) in enumerate(pairs):
        lf.set_ghost_pairs([[i, j]], n == 0)          # (the primary path rides with the first pair)
        lf.set_ghost_accumulate(n > 0)
        lf.trace_ghosts(SPP, KEY)
        assert lf.march_fix_bits() == fix
    summed = lf.read_buffer(pkg.GHOST_BUFFER).copy()
    lf.set_ghost_accumulate(False)
    assert np.array_equal(summed, whole)
    # ... and of the three single-light frames
    lf.set_ghost_pairs(None, True)
    total = np.zeros_like(whole)
    for l in lights:
        _setup(pkg, lf, asph, mask, [l])
        f, _ = _frame(pkg, lf)
        assert lf.march_fix_bits() == fix
        total += f
    assert np.array_equal(total, whole)


def test_two_contexts_reproduce_the_frame_by_rows_and_by_blocks(pkg, lf, asph, mask):
    _setup(pkg, lf, asph, mask, [SUN, LAMP])
    whole, cnt = _frame(pkg, lf)
    others = [pkg.LensFlare(0), pkg.LensFlare(0)]
    try:
        for deal in ("rows", "blocks"):
            parts, cs = [], []
            for r, ctx in enumerate(others):
                _setup(pkg, ctx, asph, mask, [SUN, LAMP])
                if deal == "rows":
                    ctx.set_row_interleave(r, 2)
                else:
                    ctx.set_block_deal(r, 2)
                f, c = _frame(pkg, ctx)
                parts.append(f); cs.append(c)
            yy, xx = np.mgrid[0:H, 0:W]
            own0 = ((yy >> 3) % 2 == 0) if deal == "rows" else (((yy >> 6) * ((W + 63) >> 6) + (xx >> 6)) % 2 == 0)
            joined = np.where(own0[..., None], parts[0], parts[1])
            assert np.array_equal(joined, whole), deal
            for name in cnt:
                assert cs[0][name] + cs[1][name] == cnt[name], (deal, name)
    finally:
        for ctx in others:
            ctx.close()


def test_occlusion_with_nothing_in_the_way_changes_no_bit(pkg, lf, asph, mask):
    _setup(pkg, lf, asph, mask, [SUN, LAMP, PANEL])
    lf.set_camera(np.eye(3).reshape(-1), [0.0, 0.0, 0.0], 40.0, 27.0)
    off, c_off = _frame(pkg, lf)
    lf.set_scene([(0.0, 0.0, 50.0, 1.0, "d", 0.5, 0.5, 0.5)], [], [])      # a ball BEHIND the camera
    lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_LIGHT)
    lf.set_ghost_occlusion(True, 0.001)
    try:
        on, c_on = _frame(pkg, lf)
        stats = lf.ghost_occlusion_stats()
    finally:
        lf.set_ghost_occlusion(False)
        lf.set_ghost_occlusion_reach(pkg.OCCLUSION_REACH_SKY)
    assert np.array_equal(on, off) and c_on == c_off and off.max() > 0
    assert stats["tested"] > 0 and stats["blocked"] == 0


# ---- routing --------------------------------------------------------------------------------------------------------------
def test_routing(pkg, lf, asph, plain, mask):
    _setup(pkg, lf, asph, mask)
    lf.timing_enable(True)
    lf.timing_reset()
    _frame(pkg, lf)
    assert lf.cull_reason() == "aspheric" and not lf.cull_info()["culled"]
    assert lf.timing_get("march")[0] == 1 and lf.timing_get("cull_prepass")[0] == 0 and lf.timing_get("cull_audit")[0] == 0
    # the lens camera's scene image refuses the lens
    lf.set_camera(np.eye(3).reshape(-1), [0.0, 0.0, 0.0], 40.0, 20.0)
    lf.set_jitter_counter(7)
    lf.set_scene([(0.0, 0.0, 0.0, 50.0, "e", 1.0, 1.0, 1.0)], [], [])
    lf.set_lens_camera(1, 0.001, 0.0)
    try:
        with pytest.raises(pkg.LensFlareError) as e:
            lf.render_scene_term()
        assert e.value.status == LF_ERR_UNSUPPORTED and "aspheric" in str(e.value)
    finally:
        lf.set_lens_camera(0)
    # aspheres set and cleared again: the kernels, the launch counts and the frame of a context that never saw one
    fresh = pkg.LensFlare(0)
    try:
        frames, launches = [], []
        for ctx, dance in ((fresh, False), (lf, True)):
            _setup(pkg, ctx, plain, mask)
            if dance:
                ctx.set_lens_aspheres(asph["aspheres"]["conic"], asph["aspheres"]["coef"])
                assert ctx.lens_aspheres()["n_aspheric"] == 2
                ctx.set_lens_aspheres(None)
                assert ctx.lens_aspheres()["n_aspheric"] == 0
            ctx.timing_enable(True)
            ctx.timing_reset()
            f, c = _frame(pkg, ctx)
            frames.append((f, c, ctx.cull_reason()))
            launches.append({k: ctx.timing_get(k)[0] for k in ("march", "cull_prepass", "cull_audit", "cull_cache_build")})
        assert launches[0] == launches[1] and frames[0][2] == frames[1][2] != "aspheric"
        assert np.array_equal(frames[0][0], frames[1][0]) and frames[0][1] == frames[1][1]
    finally:
        fresh.close()
        lf.timing_enable(False)


def test_the_terms_matter(pkg, lf, asph, plain, mask):
    _setup(pkg, lf, asph, mask)
    a, _ = _frame(pkg, lf)
    _setup(pkg, lf, plain, mask)                      # the same file with its asphere lines dropped
    b, _ = _frame(pkg, lf)
    lit = (a > 0) | (b > 0)
    assert lit.sum() > 1000
    assert (a != b)[lit].mean() > 0.10


# ---- the setter, the getter, the C parser (they need a context) -----------------------------------------------------------
def test_setter_getter_and_parsers(pkg, lf, asph, plain, mask, tmp_path):
    _setup(pkg, lf, plain, mask)
    n = plain["n"]
    conic = np.zeros(n, np.float32); coef = np.zeros((2, n), np.float32)

    def refused(kap, a, word):
        with pytest.raises(pkg.LensFlareError) as e:
            lf.set_lens_aspheres(kap, a)
        assert e.value.status == LF_ERR_INVALID and word in str(e.value), str(e.value)

    bad = conic.copy(); bad[3] = np.nan
    refused(bad, coef, "interface 3")
    bad = coef.copy(); bad[1, 7] = np.inf
    refused(conic, bad, "interface 7")
    bad = conic.copy(); bad[plain["stop"]] = -1.0
    refused(bad, coef, "stop")
    refused(conic, np.zeros((7, n), np.float32), "n_coef")
    bad = conic.copy(); bad[4] = 1.5                  # R = 12.75, h = 9: (1 + kappa) c^2 h^2 = 1.25
    refused(bad, coef, "interface 4")
    assert lf.lens_aspheres()["n_aspheric"] == 0      # a refusal leaves the state
    # an all-zero record is no asphere: today's kernels
    lf.set_lens_aspheres(conic, coef)
    assert lf.lens_aspheres()["n_aspheric"] == 0
    _frame(pkg, lf)
    assert lf.cull_reason() != "aspheric"
    # the getter returns what was set; lf_focus_lens keeps it, lf_set_lens clears it
    lf.set_lens_aspheres(asph["aspheres"]["conic"], asph["aspheres"]["coef"])
    g = lf.lens_aspheres()
    assert g["n_aspheric"] == 2 and np.array_equal(g["conic"], asph["aspheres"]["conic"]) and np.array_equal(g["coef"], asph["aspheres"]["coef"])
    info = lf.lens_info()
    lf.focus_lens(4000.0)
    assert lf.lens_aspheres()["n_aspheric"] == 2
    assert lf.lens_info()["efl_mm"] == info["efl_mm"]                 # no r^2 term: the paraxial lens is unchanged
    lf.set_lens(plain)
    assert lf.lens_aspheres()["n_aspheric"] == 0 and info["efl_mm"] == lf.lens_info()["efl_mm"]
    # the C parser gives the Python parser's arrays for the shipped file
    lf.load_lens_file(os.path.join(ROOT, "lens-flare_amd", "data", "dgauss11_asph.lens"))
    g = lf.lens_aspheres()
    assert np.array_equal(g["conic"], asph["aspheres"]["conic"]) and np.array_equal(g["coef"], asph["aspheres"]["coef"])
    src = open(os.path.join(ROOT, "lens-flare_amd", "data", "dgauss11.lens")).read()
    for tail in ("asphere 2\n", "asphere 11 0 1e-6\n", "asphere 2 0 1 2 3 4 5 6 7\n", "asphere 5 -1\n"):
        p = tmp_path / "bad.lens"
        p.write_text(src + tail)
        with pytest.raises(pkg.LensFlareError):
            lf.load_lens_file(str(p))
