"""The lens camera of the scene term under films (lf_set_lens_coatings) and the bilinear stop (lf_set_mask_filter)
against the INDEPENDENT float64 tracer, which follows both since it learnt lfo.g64_set_films / g64_set_mask_filter
(oracle/lf_geo_f64.c; pinned on the CPU by tests/test_geo_f64_films_cpu.py).  tests/test_gpu_lens_camera.py renders the
bare lens under the nearest texel only, so scene_pixel<SOFT, LENS, FILT>, k_scene_lens<SOFT, FILT>, their dispatch and
the primary table's per-wavelength film constants had no pixel behind them; here:

  a. frames (coated | bilinear | both, modes 1 and 2, a hard-edged and a smooth mask) at the bars of
     test_lens_frame_against_the_independent_float64_tracer, with the allowance capped and with the proof that the
     comparison tells each variant from its neighbour;
  b. the calibrated exposure against the tracer's own on-axis weights;
  c. lf_generate_lens_rays ray by ray through the real double Gauss, on and off the axis, three wavelengths;
  d. the compacted kernel = the per-lane kernel, bit for bit, under every variant;
  e. one ghost frame per feature against g64_trace at test_gpu_march_f64.py's bar.

The float32 oracle follows neither feature and is not used here."""
import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo
from test_geo_rays_vs_f64 import DIR_TOL, POS_TOL_MM, W_TOL
from test_gpu_lens_camera import KEY, LIGHTS, SPHERES, TRIS, compose, look_at, setup_scene_frame
from test_gpu_march_f64 import _check_against_f64

pytestmark = pytest.mark.gpu

W, H, NS, WPM = 48, 32, 16, 0.004          # the existing float64 lens-frame test's shape: strata, sub-cells, several wave tiles
POS = [0.3, 0.2, 1.0]
C2W = look_at(POS, [0.0, -0.2, -5.5])
VARIANTS = [(True, False), (False, True), (True, True)]          # (coated, bilinear)
IDS = ["coated-nearest", "bare-bilinear", "coated-bilinear"]
ALLOWANCE_CAP = 1e-3                       # of the frame's summed value


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture()
def lf(pkg):
    ctx = pkg.LensFlare(0)
    yield ctx
    ctx.close()


def the_lens(pkg, coated):
    return pkg.load_lens_file("dgauss11_coated.lens" if coated else "dgauss11.lens")


_masks = {}


def the_mask(name):
    """pentagon: 500 x 500 hard edges (and the ring of half-open footprints around them); smooth: a coarse 16 x 16
    uniform(0.25, 1) -- every ray alive, a gentle slope everywhere: the filter changes every weight"""
    if name not in _masks:
        _masks[name] = load_texels("pentbig500_14.png") if name == "pentagon" else \
            np.random.default_rng(20261019).uniform(0.25, 1.0, (16, 16)).astype(np.float32)
    return _masks[name]


class tracer_follows:
    """the float64 tracer under films / the filter for the duration of a with block; the defaults come back whatever happens"""

    def __init__(self, lens, coated, bilinear):
        self.films, self.filt = (lens["coatings"] if coated else None), int(bilinear)

    def __enter__(self):
        lfo.g64_set_films(self.films)
        lfo.g64_set_mask_filter(self.filt)

    def __exit__(self, *exc):
        lfo.g64_set_films(None)
        lfo.g64_set_mask_filter(0)


# ---- a. frames ----------------------------------------------------------------------------------------------------
_refs = {}


def tracer_frame(pkg, coated, bilinear, mode, mask_name, z_ref):
    """(frame, fragile allowance, slope allowance) of the tracer at exposure 1, each (W H, 3): computed once per variant
    and shared.  Both allowances are composed like the frame itself.  A fragile sample may go either way in float32: it
    can add or remove its potential weight times the radiance ITS ray finds (test_gpu_lens_camera.py takes the frame's
    brightest radiance there: an upper bound of this).  Under the filter every other sample's weight can move along the
    mask's slope by its slope allowance (potential weight - weight), times the radiance that sample found."""
    k = (coated, bilinear, mode, mask_name, z_ref)
    if k in _refs:
        return _refs[k]
    lens, mask = the_lens(pkg, coated), the_mask(mask_name)
    out = np.zeros((3, W * H, 3))
    with tracer_follows(lens, coated, bilinear):
        for lam in ((1,) if mode == 1 else (0, 1, 2)):
            smp = lfo.g64_lens_samples(lens, W, H, NS, KEY, lam, np.arange(W * H), mask)
            fragile, alive = smp[..., 8] > 0, smp[..., 9] == 0
            ch = slice(None) if mode == 1 else slice(lam, lam + 1)      # mode 2: channel c is wavelength c's ray
            for i, weight in enumerate((smp[..., 6], np.where(fragile, smp[..., 7], 0.0),
                                        np.where(~fragile & alive, smp[..., 7] - smp[..., 6], 0.0))):
                part = smp.copy()
                part[..., 6] = weight
                out[i][:, ch] = compose(lens, mask, W, H, NS, C2W, POS, WPM, z_ref, 1.0, part, 6, SPHERES, TRIS, LIGHTS)[0][:, ch]
    _refs[k] = tuple(out)
    return _refs[k]


def l1(got, want):
    return float(np.abs(got - want).sum() / want.sum())


def device_frame(pkg, lf, coated, bilinear, mode, mask_name):
    lens, mask = the_lens(pkg, coated), the_mask(mask_name)
    setup_scene_frame(pkg, lf, lens, mask, W, H, NS, C2W, POS)
    lf.set_mask_filter(pkg.MASK_BILINEAR if bilinear else pkg.MASK_NEAREST)
    lf.set_lens_camera(mode, WPM, 0.0)
    lf.render_scene_term()
    info = lf.lens_camera()
    assert lf.mask_filter() == int(bilinear) and lf.lens_coatings()["n_coated"] == (8 if coated else 0)
    return lf.read_buffer(pkg.SCENE_BUFFER).reshape(-1, 3), info


# The slope allowance is capped at 1e-3 of the frame (ALLOWANCE_CAP).  The smooth mask stays under it (3.3e-4, the tracer
# alone).  The pentagon does not: its edges are one anti-aliased texel wide, a slope of up to 1 per texel, and eps_mm is
# 0.0146 of its texels -- 1.33e-3 of the frame.  So the bilinear frames are held on the smooth mask only; the pentagon under
# the filter -- the ring of half-open footprints around its edges -- is seen by items d and e below.
FRAME_CASES = [(True, False, "pentagon"), (True, False, "smooth"), (False, True, "smooth"), (True, True, "smooth")]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("coated,bilinear,mask_name", FRAME_CASES, ids=[f"{i}-{m}" for i, m in zip(
    ("coated-nearest", "coated-nearest", "bare-bilinear", "coated-bilinear"), ("pentagon", "smooth", "smooth", "smooth"))])
def test_frames_against_the_float64_tracer(pkg, lf, coated, bilinear, mode, mask_name):
    """The bars of test_lens_frame_against_the_independent_float64_tracer: 2e-3 + allowance on every value, 1e-4 +
    allowance on more than 99.5 %, 1e-4 alone on more than 99 %.  Measured on an MI355X over the eight cases: median
    deviation 1.5e-7 .. 2.8e-7, largest 9.6e-5, at most 3 of 4608 values inside the allowance; slope allowance 3.3e-4 of the
    frame (smooth mask); the frame misses its own tracer frame by 1.9e-7 .. 3.0e-7 of the summed value, the films-off
    neighbour by 0.38 .. 0.63, the filter-off neighbour by 1.8e-2 (pentagon) and 5.5e-2 (smooth)."""
    got, info = device_frame(pkg, lf, coated, bilinear, mode, mask_name)
    z_ref, e = info["entrance_pupil_z_mm"], info["exposure"]
    want, fragile, slope = (a * e for a in tracer_frame(pkg, coated, bilinear, mode, mask_name, z_ref))
    allow = fragile + slope
    print(f"{mask_name} mode {mode} coated {coated} bilinear {bilinear}: of the frame's summed value, the slope allowance is "
          f"{slope.sum() / want.sum():.2e}, the fragile samples' potential weight {fragile.sum() / want.sum():.2e}")
    assert slope.sum() < ALLOWANCE_CAP * want.sum()          # a loose allowance would hide a wrong kernel
    assert bilinear or not slope.any()
    assert (want.max(axis=-1) > 0.02).mean() > 0.5           # not a dark frame
    dev = np.abs(got - want)
    assert (dev <= 2e-3 * np.abs(want) + allow + 1e-13).all(), (dev - 2e-3 * np.abs(want) - allow).max()
    assert (dev <= 1e-4 * np.abs(want) + allow + 1e-13).mean() > 0.995
    plain = dev <= 1e-4 * np.abs(want) + 1e-13
    assert plain.mean() > 0.99, plain.mean()
    lit = want > 1e-3
    print(f"  {int(lit.sum())} lit values, median rel dev {np.median(dev[lit] / want[lit]):.2e}, max "
          f"{np.max(dev[lit & plain] / want[lit & plain]):.2e}, {int((~plain).sum())} values inside the allowance")
    # the comparison can tell this variant from its neighbours -- films off, the filter off -- under the same exposure
    # and pupil: the device's frame misses each of them by more than ten times what it misses its own by
    own = l1(got, want)
    for c2, b2 in ((not coated, bilinear), (coated, not bilinear)):
        other = l1(got, tracer_frame(pkg, c2, b2, mode, mask_name, z_ref)[0] * e)
        print(f"  summed |device - tracer| / summed tracer: own {own:.2e}, coated {c2} bilinear {b2}: {other:.2e}")
        assert other > 10.0 * own, (c2, b2, own, other)
    if mode == 2 and coated:
        # a quarter-wave film tuned for 550 nm reflects more at the C and F lines than at d: against the bare lens the
        # coated frame is TINTED, channel by channel, not only brighter -- and the device shows the tracer's tint
        bare, binfo = device_frame(pkg, lf, False, bilinear, mode, mask_name)
        wb = tracer_frame(pkg, False, bilinear, mode, mask_name, z_ref)[0] * binfo["exposure"]
        tint_dev = got.sum(axis=0) / bare.sum(axis=0)
        tint_ref = want.sum(axis=0) / wb.sum(axis=0)
        tint_dev, tint_ref = tint_dev / tint_dev[1], tint_ref / tint_ref[1]
        print(f"  channel ratios coated / bare, relative to d: device {tint_dev}, tracer {tint_ref}")
        assert abs(tint_ref[0] - 1.0) > 1e-3 and abs(tint_ref[2] - 1.0) > 1e-3
        assert np.abs(tint_dev - tint_ref).max() < 0.1 * min(abs(tint_ref[0] - 1.0), abs(tint_ref[2] - 1.0))


# ---- b. exposure --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask_name", ["pentagon", "smooth"])
@pytest.mark.parametrize("coated,bilinear", [(False, False)] + VARIANTS, ids=["bare-nearest"] + IDS)
def test_calibrated_exposure_against_the_tracer(pkg, lf, coated, bilinear, mask_name):
    """calibrate_exposure = 4096 / the summed on-axis weights over the 64 x 64 cell centres of the pupil square
    (lfo.lens_exposure's grid), the tracer's weights in the float32 oracle's place: W_TOL, the project's float32-against-
    float64 bar for ONE primary path's weight -- a mean of 4096 of them does no worse.  Measured: 8.3e-8 .. 1.2e-7."""
    lens, mask = the_lens(pkg, coated), the_mask(mask_name)
    setup_scene_frame(pkg, lf, lens, mask, W, H, NS, C2W, POS)
    lf.set_mask_filter(int(bilinear))
    lf.set_lens_camera(1, WPM, 0.0)
    got = lf.lens_camera()["exposure"]
    g = (np.float32(2.0) * (np.arange(64, dtype=np.float32) + np.float32(0.5))) / np.float32(64.0) - np.float32(1.0)
    uv = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)
    with tracer_follows(lens, coated, bilinear):
        rays = lfo.g64_lens_rays(lens, 1, np.zeros_like(uv), uv, mask)
    want = 4096.0 / rays[:, 6].sum()
    print(f"exposure {mask_name} coated {coated} bilinear {bilinear}: device {got:.9g}, tracer {want:.9g}, relative "
          f"{abs(got / want - 1.0):.2e}; {int((rays[:, 8] > 0).sum())} fragile of {int((rays[:, 9] == 0).sum())} alive rays")
    assert abs(got - want) <= W_TOL * want


# ---- c. per ray ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coated,bilinear", VARIANTS, ids=IDS)
def test_lens_rays_on_the_double_gauss_against_the_tracer(pkg, lf, coated, bilinear):
    """k_lens_rays<kVarCoat | kVarFilt | kVarCoatFilt>: a 24 x 24 pupil grid from the axis and from (3, -2) mm, all three
    wavelengths, against the tracer from the same float32 sensor and pupil points: ten curved interfaces crossed obliquely
    (the per-ray film tests know slabs and the axial ray, the per-ray filter tests a plate and ratios).  Rays the tracer
    does not call fragile have its fate; exit point, direction and weight within POS_TOL_MM, DIR_TOL and W_TOL of
    tests/test_geo_rays_vs_f64.py, the weight under the filter within W_TOL + its slope allowance / its weight.
    Measured: 6.7e-6 mm, 3.3e-7, weight 9.4e-7 (coated) and 3.0e-6 (filtered; the largest slope allowance is 1.6e-3)."""
    lens, mask = the_lens(pkg, coated), the_mask("smooth")
    lf.set_frame(64, 64)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    lf.set_mask_filter(int(bilinear))
    g = (np.arange(24) + 0.5) / 12.0 - 1.0
    uv = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2).astype(np.float32)
    worst = dict(pos=0.0, dir=0.0, w=0.0, slope=0.0)
    n_alive = n_dead = n_fragile = 0
    for xy0 in ((0.0, 0.0), (3.0, -2.0)):
        xy = np.tile(np.float32(xy0), (len(uv), 1))
        for lam in range(3):
            got = lf.generate_lens_rays(lam, xy, uv).astype(np.float64)
            with tracer_follows(lens, coated, bilinear):
                ref = lfo.g64_lens_rays(lens, lam, xy, uv, mask)
            firm = ref[:, 8] == 0
            n_fragile += int((~firm).sum())
            assert np.array_equal(got[firm, 7] == 1.0, ref[firm, 9] == 0), (xy0, lam)
            a = firm & (ref[:, 9] == 0)
            n_alive += int(a.sum())
            n_dead += int((firm & ~a).sum())
            d = got[a, 3:6] / np.linalg.norm(got[a, 3:6], axis=1)[:, None]
            e_pos = np.abs(got[a, 0:3] - ref[a, 0:3]).max(axis=1)
            e_dir = np.abs(d - ref[a, 3:6]).max(axis=1)
            e_w = np.abs(got[a, 6] - ref[a, 6]) / ref[a, 6]
            slope = (ref[a, 7] - ref[a, 6]) / ref[a, 6]
            assert bilinear or not slope.any()
            assert (e_pos <= POS_TOL_MM).all() and (e_dir <= DIR_TOL).all(), (xy0, lam, e_pos.max(), e_dir.max())
            assert (e_w <= W_TOL + slope).all(), (xy0, lam, (e_w - slope).max())
            worst = dict(pos=max(worst["pos"], e_pos.max()), dir=max(worst["dir"], e_dir.max()), w=max(worst["w"], e_w.max()),
                         slope=max(worst["slope"], slope.max()))
    print(f"coated {coated} bilinear {bilinear}: {n_alive} alive and {n_dead} blocked rays ({n_fragile} fragile skipped): worst exit "
          f"point {worst['pos']:.2e} mm, direction {worst['dir']:.2e}, weight {worst['w']:.2e} relative (largest slope allowance "
          f"{worst['slope']:.2e})")
    assert n_alive >= 100 and n_dead >= 100


# ---- d. compacted = per-lane ----------------------------------------------------------------------------------------

def _compact_frames(pkg, lf, what, Wd, Hd):
    frames, counters = [], []
    try:
        for compact, strided in ((1, 1), (0, 0), (1, 0), (0, 1)):
            lf.test_knob("scene_compact", compact)
            lf.test_knob("scene_lens_strided", strided)
            lf.set_scene_term(np.zeros((Hd, Wd, 3)))
            lf.reset_scene_counters()
            lf.render_scene_term()
            frames.append(lf.read_buffer(pkg.SCENE_BUFFER))
            counters.append(lf.scene_counters())
    finally:
        lf.test_knob("scene_compact", -1)
        lf.test_knob("scene_lens_strided", -1)
    return frames, counters


@pytest.mark.parametrize("what,coated,bilinear",
                         [(w, c, b) for w in ("delta_one_lambda", "per_wavelength") for c, b in VARIANTS] + [("area_light", True, True)])
def test_compacted_equals_per_lane_under_the_variants(pkg, lf, what, coated, bilinear):
    """test_compacted_scene_rays_equal_the_per_lane_kernel's idea under films and the filter: k_scene_lens<SOFT, FILT>
    against k_scene_term<SOFT, true> -> scene_pixel<SOFT, true, FILT>, both pixel layouts: frames and counters bit for
    bit -- so a FILT dropped by one dispatch, or film constants read differently by one kernel, cannot pass; the filtered
    frame is not the nearest one."""
    lens, mask = the_lens(pkg, coated), the_mask("pentagon")
    Wd, Hd, ns = 96, 64, 16
    pos = [0.2, 0.1, 0.8]
    setup_scene_frame(pkg, lf, lens, mask, Wd, Hd, ns, look_at(pos, [0.0, -0.2, -5.5]), pos)
    if what == "area_light":
        lf.set_sampling(8, 0.25, 0.01, 100.0)
        lf.set_scene_lights([[0.0, 2.0, 1.8, 1.5, 0.3 / 1.0, 0.8, 0.52] + [0.0] * 9,
                             [3.0, 6.0, 6.0, 5.0, 0.0, 2.5, -5.0, 0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
        lf.set_light_samples(4)
    lf.set_mask_filter(int(bilinear))
    lf.set_lens_camera(2 if what == "per_wavelength" else 1, 0.003, 0.0)
    frames, counters = _compact_frames(pkg, lf, what, Wd, Hd)
    assert (frames[0].max(axis=-1) > 1e-3).mean() > 0.1
    for k in (1, 2, 3):
        assert np.array_equal(frames[0], frames[k]), (k, np.abs(frames[0] - frames[k]).max())
        assert counters[0] == counters[k], (k, counters)
    if bilinear:
        lf.set_mask_filter(pkg.MASK_NEAREST)
        near, near_counters = _compact_frames(pkg, lf, what, Wd, Hd)
        for k in (1, 2, 3):
            assert np.array_equal(near[0], near[k]) and near_counters[0] == near_counters[k]
            assert not np.array_equal(frames[k], near[k])
        assert counters[0]["lens_left"] > near_counters[0]["lens_left"]      # the half-open footprints around the pentagon
    if coated:
        lf.set_lens_coatings(None)
        lf.set_mask_filter(int(bilinear))
        lf.set_scene_term(np.zeros((Hd, Wd, 3)))
        lf.reset_scene_counters()
        lf.render_scene_term()
        assert not np.array_equal(lf.read_buffer(pkg.SCENE_BUFFER), frames[0])
        if what != "area_light":                                             # (no adaptive early-out: the same samples)
            assert lf.scene_counters() == counters[0]                        # films never change a ray's fate


# ---- e. one ghost frame ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coated,bilinear", [(True, False), (False, True)], ids=IDS[:2])
def test_ghost_frame_against_the_float64_tracer(pkg, lf, coated, bilinear):
    """test_gpu_march_f64.py::test_dgauss_converged_pixels_within_1e4's frame -- 64 x 48, 256 spp, the pentagon, the primary
    path and all 45 pairs -- and its own check, with films or under the filter: the first time either feature's GHOST
    pixels meet an independent tracer.  Cull modes 0 and 2 -- on a frame this narrow a cull block would be too large on the
    sensor (lf_get_cull_reason: block_too_large), so mode 2 marches everything too, as that test's default mode does;
    the culled march under either feature is held to the full enumeration bit for bit by tests/test_gpu_coatings.py and
    tests/test_gpu_mask_filter.py.  The tracer marches the frame once per table the device reports (here: none).
    Measured: coated 196 lit values, largest deviation 9.9e-6, median 4.5e-7; filtered 195, 7.2e-6, 6.1e-7; none of them
    needs the allowance."""
    lens, mask = the_lens(pkg, coated), the_mask("pentagon")
    Wg, Hg, spp, key = 64, 48, 256, 0xBEEF
    sun, rad, alpha = [0.03, 0.02, -1.0], [1.0, 0.9, 0.5], 0.05
    lf.set_frame(Wg, Hg)
    lf.set_mask_filter(int(bilinear))
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    lf.set_sun(sun, rad, alpha)
    lf.set_ghost_pairs(None, True)
    refs = {}
    for cull in (0, 2):
        lf.set_march_culling(cull)
        lf.reset_counters()
        lf.trace_ghosts(spp, key)
        img, cnt, table = lf.read_buffer(pkg.GHOST_BUFFER), lf.counters(), lf.cull_table_and_block()
        print(f"ghost frame coated {coated} bilinear {bilinear} cull mode {cull}: {lf.cull_reason()}")
        assert cull != 0 or table is None
        k = None if table is None else cull
        if k not in refs:
            with tracer_follows(lens, coated, bilinear):
                refs[k] = lfo.g64_trace(lens, Wg, Hg, 0, Hg, spp, key, None, True, mask, sun, rad, alpha, n_threads=16, cull=table)
        ref, frag, c64 = refs[k]
        lit = ref >= 2e-5
        rel = _check_against_f64(img, cnt, ref, frag, c64, min_lit=150, culled=table is not None)
        print(f"  {rel.size} converged channel values, max rel {rel.max():.2e}, median {np.median(rel):.2e}; fragile + slope "
              f"allowance {frag[lit].sum() / ref[lit].sum():.2e} of their sum")
    lf.set_march_culling(1)
