"""The geometric march on the GPU against an INDEPENDENT float64 tracer (oracle/lf_geo_f64.c:
textbook sphere quadratic, vector Snell, r_s / r_p Fresnel, libm sqrt -- no code, no float32
recipe and no sqrt table in common with the bit-exact oracle), at the north star's bar: converged
pixels within 1e-4 relative.  Float32 and float64 can disagree about the fate of a ray that passes
within rounding distance of an aperture edge, a mask-texel edge or the critical angle; the tracer
bounds the weight of those rays per pixel (`frag`), and the test states how often that allowance is
needed at all.  Also here: the coherent pupil sub-cells converge to the independent estimate."""
import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo

pytestmark = pytest.mark.gpu

TOL = 1e-4
# a contribution is accumulated as 2^-36 fixed point (truncated): up to 46 paths x n_lambda
# contributions per sample can each lose 1.5e-11, i.e. <= 2e-9 per pixel -- the stated floor keeps
# that below TOL / 10
FLOOR = 2e-5


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="module")
def lf(pkg):
    ctx = pkg.LensFlare(0)
    yield ctx
    ctx.close()


def _gpu_frame(pkg, lf, lens, W, H, spp, key, mask, sun, rad, alpha, sub_bits=None, pairs=None):
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    lf.set_sun(sun, rad, alpha)
    lf.set_ghost_pairs(pairs, True)
    lf.set_pupil_subcells(pkg.DEFAULT_SUBCELL_BITS if sub_bits is None else sub_bits)
    lf.reset_counters()
    lf.trace_ghosts(spp, key)
    img = lf.read_buffer(pkg.GHOST_BUFFER)
    cnt = lf.counters()
    lf.set_pupil_subcells(pkg.DEFAULT_SUBCELL_BITS)
    return img, cnt


def _check_against_f64(img, cnt, ref, frag, c64, min_lit, median_bar=2e-6, culled=False, hit_light_slack=0):
    """hit_light_slack: (ray, light) pairs whose lit-or-unlit decision the tracer calls undecidable at float32 accuracy beside the
    fragile rays -- the edge band of a rectangle (light_edge_pairs, tests/test_gpu_lights_f64.py) -- allowed on rays_hit_light only"""
    assert c64["rays_launched"] == cnt["rays_launched"]
    lit = ref >= FLOOR
    assert lit.sum() >= min_lit, "the test frame must have converged pixels above the floor"
    rel = np.abs(img - ref)[lit] / ref[lit]
    # the bar, with the fragile rays' weight as the only allowance
    assert np.all(np.abs(img - ref)[lit] <= TOL * ref[lit] + 1.05 * frag[lit]), rel.max()
    # How much of the allowance is actually consumed: for every lit value EITHER the raw deviation is within
    # 1e-4 OR it is within the summed potential weight of that pixel's fragile rays (frag; the 5 % on top
    # covers the float32 rounding of those weights themselves).  The histogram of deviation / frag over the
    # values that need the allowance goes to the test's output.
    dev = np.abs(img - ref)[lit]
    over = dev > TOL * ref[lit]
    if over.any():
        f = frag[lit][over]
        assert np.all(f > 0), "a value outside 1e-4 whose pixel has no fragile ray at all"
        ratio = dev[over] / f
        assert ratio.max() <= 1.05, ratio.max()
        hist, _ = np.histogram(ratio, bins=[0, 0.25, 0.5, 0.75, 1.0, 1.05])
        print(f"  allowance: {int(over.sum())} of {int(lit.sum())} lit values are outside 1e-4; deviation / (summed weight "
              f"of the pixel's fragile rays) in [0,.25) [.25,.5) [.5,.75) [.75,1) [1,1.05]: {hist.tolist()}, max {ratio.max():.3f}; "
              f"largest raw deviation {rel.max():.2e}")
    elif rel.size:
        print(f"  allowance: none of {int(lit.sum())} lit values needs it (largest raw deviation {rel.max():.2e})")
    # ... and that allowance is the exception, not the rule
    if rel.size:
        assert (rel <= TOL).mean() >= 0.98, (rel <= TOL).mean()
        assert np.median(rel) < median_bar, np.median(rel)
    # dim pixels: absolute agreement at the accumulation quantum
    assert np.all(np.abs(img - ref)[~lit] <= TOL * FLOOR + 1.05 * frag[~lit])
    # ray fates agree except for the fragile rays
    n_frag = c64["rays_fragile"]
    # (fragile rays are the rare ones -- 0.3 % of a full enumeration; a culled launch starts few rays besides those
    # that pass near an edge of something, so there they are a larger part of what is counted: 1.3 % on the c3 band)
    assert n_frag < (5e-2 if culled else 1e-2) * c64["rays_launched"]
    for name in ("rays_clipped_stop", "rays_vignetted", "rays_tir", "rays_reached_scene", "rays_hit_light"):
        assert abs(c64[name] - cnt[name]) <= n_frag + (hit_light_slack if name == "rays_hit_light" else 0), (name, c64[name], cnt[name])
    assert abs(c64["surface_events"] - cnt["surface_events"]) <= 30 * n_frag
    return rel


def test_dgauss_converged_pixels_within_1e4(pkg, lf):
    """64x48, 256 spp, double-Gauss, primary + all 45 pairs, 3 wavelengths, pentagon mask."""
    lens = pkg.load_lens_file("dgauss11.lens")
    mask = load_texels("pentbig500_14.png")
    W, H, spp, key = 64, 48, 256, 0xBEEF
    sun, rad, alpha = [0.03, 0.02, -1.0], [1.0, 0.9, 0.5], 0.05
    img, cnt = _gpu_frame(pkg, lf, lens, W, H, spp, key, mask, sun, rad, alpha)
    ref, frag, c64 = lfo.g64_trace(lens, W, H, 0, H, spp, key, None, True, mask, sun, rad, alpha,
                                   n_threads=16, cull=lf.cull_table_and_block())
    rel = _check_against_f64(img, cnt, ref, frag, c64, min_lit=150)
    print(f"dgauss: {rel.size} converged channel values, max rel {rel.max():.2e}, median {np.median(rel):.2e}")


def test_thin_lens_converged_pixels_within_1e4(pkg, lf):
    """BASELINE configs[0]'s lens (2 spherical surfaces, no stop), one ghost pair + primary."""
    lens = pkg.load_lens_file("thinlens.lens")
    mask = np.ones((8, 8), np.float32)
    W, H, spp, key = 64, 48, 256, 0x7117
    sun, rad, alpha = [0.02, -0.01, -1.0], [1.0, 1.0, 1.0], 0.1
    img, cnt = _gpu_frame(pkg, lf, lens, W, H, spp, key, mask, sun, rad, alpha)
    ref, frag, c64 = lfo.g64_trace(lens, W, H, 0, H, spp, key, None, True, mask, sun, rad, alpha,
                                   n_threads=16, cull=lf.cull_table_and_block())
    rel = _check_against_f64(img, cnt, ref, frag, c64, min_lit=1000)
    print(f"thin lens: {rel.size} converged channel values, max rel {rel.max():.2e}")


def test_eight_wavelengths_within_1e4(pkg, lf):
    """C5's 8 wavelengths with RGB weights, the same bar."""
    lens8 = pkg.load_lens_file("dgauss11_8lambda.lens")   # 2-term Cauchy fit through C, d, F
    w8, _ = pkg.spectral_weights(lens8["lambda_nm"])
    mask = load_texels("pentbig500_14.png")
    W, H, spp, key = 48, 32, 144, 0x8888
    sun, rad, alpha = [0.02, 0.03, -1.0], [1.0, 0.9, 0.5], 0.05
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens8)
    lf.set_lambda_rgb(w8)
    lf.set_sun(sun, rad, alpha)
    lf.set_ghost_pairs(None, True)
    lf.reset_counters()
    lf.trace_ghosts(spp, key)
    img, cnt = lf.read_buffer(pkg.GHOST_BUFFER), lf.counters()
    ref, frag, c64 = lfo.g64_trace(lens8, W, H, 0, H, spp, key, None, True, mask, sun, rad, alpha,
                                   n_threads=16, lambda_rgb=w8, cull=lf.cull_table_and_block())
    _check_against_f64(img, cnt, ref, frag, c64, min_lit=50)


def test_pupil_subcells_converge_to_the_independent_estimate(pkg, lf):
    """All 64 pixels of a wave tile share one pupil sub-cell per sample (coherent fate at the mask):
    per pixel that is still a uniform draw from the stratum, so the estimator is unbiased, but the
    noise is correlated inside a tile.  Check against the fully independent estimator (bits = 0):
    the means over 12 keys agree within the Monte-Carlo error per pixel and in total, and the two
    estimators have the same per-pixel variance (the correlation does not cost variance)."""
    lens = pkg.load_lens_file("dgauss11.lens")
    mask = load_texels("pentbig500_14.png")
    W, H, spp = 48, 32, 64
    sun, rad, alpha = [0.03, 0.02, -1.0], [1.0, 0.9, 0.5], 0.05
    keys = [0x1000 + 17 * k for k in range(12)]
    runs = {}
    # (the SHIPPED specification -- pkg.DEFAULT_SUBCELL_BITS sub-cells under the default tile stride, ADVICE r4 --
    # against the independent estimator; 4 bits, the value this test used through round 4, is checked the same way)
    for bits in (pkg.DEFAULT_SUBCELL_BITS, 4, 0):
        runs[bits] = np.stack([_gpu_frame(pkg, lf, lens, W, H, spp, k, mask, sun, rad, alpha,
                                          sub_bits=bits)[0].sum(axis=2) for k in keys])
    b = runs[0]
    for bits in (4, pkg.DEFAULT_SUBCELL_BITS):
        a = runs[bits]
        ma, mb = a.mean(axis=0), b.mean(axis=0)
        se = np.sqrt((a.var(axis=0, ddof=1) + b.var(axis=0, ddof=1)) / len(keys))
        lit = (ma + mb) > 2 * FLOOR
        z = (ma - mb)[lit] / np.maximum(se[lit], 1e-12)
        assert lit.sum() > 30 and np.abs(z).max() < 6.0 and (np.abs(z) < 3.0).mean() > 0.95 and abs(z.mean()) < 0.35, \
            (bits, np.abs(z).max(), (np.abs(z) < 3).mean(), z.mean())
    a = runs[pkg.DEFAULT_SUBCELL_BITS]
    ma, mb = a.mean(axis=0), b.mean(axis=0)
    se = np.sqrt((a.var(axis=0, ddof=1) + b.var(axis=0, ddof=1)) / len(keys))
    lit = (ma + mb) > 2 * FLOOR
    assert lit.sum() > 30
    z = (ma - mb)[lit] / np.maximum(se[lit], 1e-12)
    assert np.abs(z).max() < 6.0 and (np.abs(z) < 3.0).mean() > 0.95, (np.abs(z).max(), (np.abs(z) < 3).mean())
    assert abs(z.mean()) < 0.35, z.mean()                       # no systematic offset
    # whole-image flux: correlated noise does not average out inside a tile, so compare the frame
    # totals with their own run-to-run scatter
    ta, tb = a.sum(axis=(1, 2)), b.sum(axis=(1, 2))
    s_tot = np.sqrt((ta.var(ddof=1) + tb.var(ddof=1)) / len(keys))
    assert abs(ta.mean() - tb.mean()) < 4.0 * s_tot
    # per-pixel variance: the same estimator quality
    ratio = np.median(a.var(axis=0, ddof=1)[lit] / np.maximum(b.var(axis=0, ddof=1)[lit], 1e-30))
    assert 0.6 < ratio < 1.6, ratio
    # ... and both converge to the float64 tracer's expectation (common key: same sample points)
    ref, frag, _ = lfo.g64_trace(lens, W, H, 0, H, spp, keys[0], None, True, mask, sun, rad, alpha,
                                 n_threads=16, sub_bits=0)
    img0, _ = _gpu_frame(pkg, lf, lens, W, H, spp, keys[0], mask, sun, rad, alpha, sub_bits=0)
    litp = ref >= FLOOR
    assert np.all(np.abs(img0 - ref)[litp] <= TOL * ref[litp] + 1.05 * frag[litp])


# ---- the independent check at BENCH size ----------------------------------------------------------------
SUN_NS = (0.521445, 0.517156)


def _host_threads():
    import os
    return int(os.environ.get("LF_LONG_THREADS", os.cpu_count() or 8))


def _band_against_f64(pkg, lf, lens, W, H, y0, y1, spp, key, mask, lambda_rgb=None, min_lit=200, median_bar=2e-6,
                      x_window=None, causes=None):
    import os
    efl = pkg.paraxial_efl(lens)
    sun = [(SUN_NS[0] - 0.5) * lens["sensor_width_mm"] / efl, (SUN_NS[1] - 0.5) * lens["sensor_width_mm"] * H / W / efl, -1.0]
    rad, alpha = [1.0, 0.9, 0.5], 0.05
    lf.set_frame(W, H)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    if lambda_rgb is not None:
        lf.set_lambda_rgb(lambda_rgb)
    lf.set_sun(sun, rad, alpha)
    lf.set_ghost_pairs(None, True)
    lf.set_band(y0, y1)                 # the band alone: its own ray budget and counters
    lf.reset_counters()
    lf.trace_ghosts(spp, key)
    img = lf.read_tile(pkg.GHOST_BUFFER, 0, y0, W, y1)
    cnt = lf.counters()
    lf.set_band(0, H)
    if x_window == "auto":
        # the columns where the DEVICE's band holds anything at all (>= FLOOR / 4), +- 16: outside them nothing is lit in
        # the device's frame -- and a frame that were dark where the tracer's is lit is what the whole-frame record
        # (LF_LONG_CHECKS, profiles/r06_f64_whole_frame.log) would show
        cols = np.where((img >= 0.25 * FLOOR).any(axis=(0, 2)))[0]
        x_window = (max(0, int(cols.min()) - 16), min(W, int(cols.max()) + 17)) if cols.size else (W // 2 - 32, W // 2 + 32)
        outside = np.ones(W, bool)
        outside[x_window[0]:x_window[1]] = False
        assert not (img[:, outside] >= 0.25 * FLOOR).any()
        print(f"  rows {y0}..{y1}: columns {x_window[0]}..{x_window[1]} of {W} traced in float64", flush=True)
    if x_window is not None:
        # columns [x0, x1) only: the device marched the whole band (cheap), the float64 tracer the window;
        # pixels are compared inside it, the ray-fate counters (a whole-band property) are not
        lfo.g64_set_x_window(*x_window)
    try:
        ref, frag, c64 = lfo.g64_trace(lens, W, H, y0, y1, spp, key, None, True, mask, sun, rad, alpha,
                                       n_threads=_host_threads(), lambda_rgb=lambda_rgb, causes=causes is not None,
                                       cull=lf.cull_table_and_block())   # (pixels: the full enumeration's; counters: the rays the device started)
    finally:
        lfo.g64_set_x_window()
    ref, frag = ref[y0:y1], frag[y0:y1]
    if x_window is not None:
        x0, x1 = x_window
        img, ref, frag = img[:, x0:x1], ref[:, x0:x1], frag[:, x0:x1]
        lit = ref >= FLOOR
        assert lit.sum() >= min_lit
        dev = np.abs(img - ref)
        assert np.all(dev[lit] <= TOL * ref[lit] + 1.05 * frag[lit]), (dev[lit] / ref[lit]).max()
        assert np.all(dev[~lit] <= TOL * FLOOR + 1.05 * frag[~lit])
        rel = dev[lit] / ref[lit]
        assert rel.size == 0 or ((rel <= TOL).mean() >= 0.98 and np.median(rel) < median_bar)
        over = dev[lit] > TOL * ref[lit]
        if over.any():
            ratio = dev[lit][over] / frag[lit][over]
            assert ratio.max() <= 1.05
            hist, _ = np.histogram(ratio, bins=[0, 0.25, 0.5, 0.75, 1.0, 1.05])
            print(f"  allowance: {int(over.sum())} of {int(lit.sum())} lit values outside 1e-4; deviation / fragile weight "
                  f"histogram {hist.tolist()}, max {ratio.max():.3f}; largest raw deviation {rel.max():.2e}")
        if causes is not None:
            _tally_causes(causes, lit, lit & (dev > TOL * ref), dev, frag, rel, lfo.g64_last_causes[y0:y1, x0:x1])
        return rel, int(over.sum()), c64
    rel = _check_against_f64(img, cnt, ref, frag, c64, min_lit=min_lit, median_bar=median_bar, culled=lf.cull_info()["culled"])
    lit = ref >= FLOOR
    dev = np.abs(img - ref)
    over = lit & (dev > TOL * ref)
    needed = int(over.sum())
    if causes is not None:
        _tally_causes(causes, lit, over, dev, frag, rel, lfo.g64_last_causes[y0:y1])
    return rel, needed, c64


def _tally_causes(causes, lit, over, dev, frag, rel, by):
    """the values that needed the fragile-ray allowance: how much of it, the largest raw deviation, and WHAT made their
    rays fragile (per value: the cause that carries most of its pixel's fragile weight; `by`: rows x columns x cause)"""
    needed = int(over.sum())
    causes["values"] = causes.get("values", 0) + int(lit.sum())
    causes["needed"] = causes.get("needed", 0) + needed
    causes["max_raw_rel"] = max(causes.get("max_raw_rel", 0.0), float(rel.max()) if rel.size else 0.0)
    if needed:
        ratio = dev[over] / frag[over]
        hist, _ = np.histogram(ratio, bins=[0, 0.25, 0.5, 0.75, 1.0, 1.05])
        causes["ratio_hist"] = (np.asarray(causes.get("ratio_hist", [0] * 5)) + hist).tolist()
        causes["max_ratio"] = max(causes.get("max_ratio", 0.0), float(ratio.max()))
        dom = by.argmax(axis=2)[..., None].repeat(3, axis=2)[over]
        for k, name in enumerate(lfo.G64_CAUSES):
            causes[name] = causes.get(name, 0) + int((dom == k).sum())


def test_c3_band_at_full_spp_against_the_independent_tracer(pkg, lf):
    """The benchmark frame itself -- 1920x1080, 256 spp, primary + 45 pairs x 3 wavelengths -- on the
    8-row tile row through the sun (5e8 rays): every pixel within 1e-4 of the float64 tracer up to the
    fragile rays' weight, ray fates equal up to the number of fragile rays."""
    lens = pkg.load_lens_file("dgauss11.lens")
    mask = load_texels("pentbig500_14.png")
    W, H, spp, key = 1920, 1080, 256, 0x1e45f1a4e
    y0 = (int(SUN_NS[1] * H) // 8) * 8
    rel, needed, c64 = _band_against_f64(pkg, lf, lens, W, H, y0, y0 + 8, spp, key, mask, min_lit=2000)
    print(f"c3 band rows {y0}..{y0 + 8}: {rel.size} lit channel values, max rel {rel.max():.2e}, median "
          f"{np.median(rel):.2e}; the fragile-ray allowance was needed by {needed} of them "
          f"({c64['rays_fragile']} fragile rays of {c64['rays_launched']})")


def test_c3_lit_band_of_40_rows_against_the_independent_tracer(pkg, lf):
    """a 40-row band of the benchmark frame across the sun (the rows where most of the
    frame's light is), 256 spp, all 46 paths x 3 wavelengths -- 2.7e9 rays through the float64 tracer on the
    host's cores (about a minute on the GPU box's 256; the band shrinks on a smaller host) -- in the
    DEFAULT run, so that the driver's record carries it and not a builder's log."""
    import os
    import time
    lens = pkg.load_lens_file("dgauss11.lens")
    mask = load_texels("pentbig500_14.png")
    W, H, spp, key = 1920, 1080, 256, 0x1e45f1a4e
    cores = _host_threads()
    rows = 40 if cores >= 128 else 16 if cores >= 32 else 8
    y0 = ((int(SUN_NS[1] * H) - rows // 2) // 8) * 8
    t0 = time.time()
    rel, needed, c64 = _band_against_f64(pkg, lf, lens, W, H, y0, y0 + rows, spp, key, mask, min_lit=2000)
    print(f"c3 band rows {y0}..{y0 + rows} ({cores} host threads, {time.time() - t0:.0f} s): {rel.size} lit channel values, "
          f"max rel {rel.max():.2e}, median {np.median(rel):.2e}; allowance needed by {needed} "
          f"({c64['rays_fragile']} fragile rays of {c64['rays_launched']})")


def test_c3_every_lit_band_against_the_independent_tracer(pkg, lf):
    """every lit value of the benchmark frame in the DEFAULT run.  The whole-frame comparison
    (profiles/r05_f64_whole_frame.log, r06_f64_whole_frame.log) finds them in rows 400..720 -- 159 000 values in EIGHT
    40-row bands, not the four (560..720) the review named from the log's second half -- and in each band only in the few
    hundred columns around the sun's image: the float64 tracer marches exactly those columns (where the device's band holds
    anything at all, +- 16 px; a quarter of a minute per band instead of a minute), at the full 256 spp, with what the
    driver's record should show: how many values needed the fragile-ray allowance, how much of it (histogram of deviation
    / fragile weight), the largest raw deviation, and the cause of the fragility -- the rim of a clear aperture, the edge
    of a mask texel (the stop's mask is looked up nearest-texel: a hard edge at every texel), the critical angle, a
    grazing miss.  (Ray-fate counters are a whole-band property: test_c3_lit_band_of_40_rows compares them.)"""
    import json
    import time
    lens = pkg.load_lens_file("dgauss11.lens")
    mask = load_texels("pentbig500_14.png")
    W, H, spp, key = 1920, 1080, 256, 0x1e45f1a4e
    cores = _host_threads()
    rows = 40 if cores >= 128 else 8
    causes = {}
    t0 = time.time()
    for y0 in range(400, 720, 40):
        rel, needed, c64 = _band_against_f64(pkg, lf, lens, W, H, y0, y0 + rows, spp, key, mask, min_lit=0, median_bar=1e-5,
                                             causes=causes, x_window="auto")
        print(f"c3 rows {y0}..{y0 + rows}: {rel.size} lit values, max rel {rel.max() if rel.size else 0:.2e}, allowance needed by "
              f"{needed}, {c64['rays_fragile']} fragile rays of {c64['rays_launched']} ({time.time() - t0:.0f} s)", flush=True)
    print("LIT BANDS:", json.dumps(causes), flush=True)
    assert causes["values"] > (120000 if rows == 40 else 10000)
    assert causes["needed"] < 1e-3 * causes["values"] and causes.get("max_ratio", 0.0) <= 1.05


def test_c5_tile_row_at_its_full_1024_spp_against_the_independent_tracer(pkg, lf):
    """C5 at the sample count BASELINE.json names -- 4K, 8 wavelengths, 1024 spp -- on
    the 8-row tile row through the sun, the 960 columns around the sun's image (2.9e9 rays in float64; the
    window shrinks on a smaller host), in the DEFAULT run."""
    import time
    lens8 = pkg.load_lens_file("dgauss11_8lambda.lens")
    w8, _ = pkg.spectral_weights(lens8["lambda_nm"])
    mask = load_texels("pentbig500_14.png")
    W, H, spp, key = 3840, 2160, 1024, 0xC5C5
    cores = _host_threads()
    half = 480 if cores >= 128 else 160 if cores >= 32 else 48
    y0 = (int(SUN_NS[1] * H) // 8) * 8
    cx = int(SUN_NS[0] * W)
    t0 = time.time()
    rel, needed, c64 = _band_against_f64(pkg, lf, lens8, W, H, y0, y0 + 8, spp, key, mask, lambda_rgb=w8,
                                         min_lit=40 * half // 10, x_window=(cx - half, cx + half))
    print(f"c5 tile row {y0}..{y0 + 8}, columns {cx - half}..{cx + half} at {spp} spp ({cores} host threads, "
          f"{time.time() - t0:.0f} s): {rel.size} lit channel values, max rel {rel.max():.2e}, median {np.median(rel):.2e}; "
          f"allowance needed by {needed} ({c64['rays_fragile']} fragile rays of {c64['rays_launched']})")


def _c5_band(pkg, lf, spp, rows_per_call=16):
    lens8 = pkg.load_lens_file("dgauss11_8lambda.lens")   # 2-term Cauchy fit through C, d, F
    w8, _ = pkg.spectral_weights(lens8["lambda_nm"])
    mask = load_texels("pentbig500_14.png")
    W, H, key = 3840, 2160, 0xC5C5
    y_top = (int(SUN_NS[1] * H) // 8) * 8 - 8
    for y0 in range(y_top, y_top + 16, rows_per_call):   # (sub-bands: a progress line every few minutes)
        y1 = y0 + rows_per_call
        rel, needed, c64 = _band_against_f64(pkg, lf, lens8, W, H, y0, y1, spp, key, mask, lambda_rgb=w8,
                                             min_lit=2000 * rows_per_call // 16)
        print(f"c5 band rows {y0}..{y1} at {spp} spp: {rel.size} lit channel values, max rel {rel.max():.2e}, median "
              f"{np.median(rel):.2e}; allowance needed by {needed} ({c64['rays_fragile']} fragile rays of "
              f"{c64['rays_launched']})", flush=True)


def test_c5_band_of_the_4k_frame_against_the_independent_tracer(pkg, lf):
    """C5's frame size and its 8 wavelengths, a 16-row band through the sun at 64 of the 1024 spp
    (both sides evaluate the same samples, so the sample count only sets the coverage: 1.4e9 rays)."""
    _c5_band(pkg, lf, 64)


@pytest.mark.skipif(__import__("os").environ.get("LF_LONG_CHECKS") != "1",
                    reason="minutes of host time on a many-core box: LF_LONG_CHECKS=1 (record: profiles/r05_f64_c5_band.log)")
def test_c5_band_at_full_spp_against_the_independent_tracer(pkg, lf):
    """The same band of the C5 frame at its FULL 1024 spp (2.3e10 rays: a third of the whole c3 frame)."""
    _c5_band(pkg, lf, 1024, rows_per_call=4)


@pytest.mark.skipif(__import__("os").environ.get("LF_LONG_CHECKS") != "1",
                    reason="27 minutes of the box's 16 host CPUs: LF_LONG_CHECKS=1, in two calls (LF_LONG_Y0 / LF_LONG_Y1); record: profiles/r05_f64_whole_frame.log")
def test_c3_whole_frame_against_the_independent_tracer(pkg, lf):
    """The WHOLE benchmark frame -- 1920x1080, 256 spp, primary + 45 pairs x 3 wavelengths, 7.3e10 rays --
    band by band against the float64 tracer, each band to the same bar as the 8-row test above.  Not
    part of the default run (the tracer needs ~10 core-hours); run once per round on the GPU box's host
    cores and its summary kept under profiles/."""
    import json
    import os
    import time
    lens = pkg.load_lens_file("dgauss11.lens")
    mask = load_texels("pentbig500_14.png")
    W, H, spp, key = 1920, 1080, 256, 0x1e45f1a4e
    rows = int(os.environ.get("LF_LONG_BAND_ROWS", "40"))
    y_lo, y_hi = int(os.environ.get("LF_LONG_Y0", "0")), int(os.environ.get("LF_LONG_Y1", str(H)))
    tot = dict(values=0, needed=0, fragile=0, rays=0, max_rel=0.0, bands=0, lit_bands=0)
    meds = []
    t0 = time.time()
    for y0 in range(y_lo, y_hi, rows):
        y1 = min(y0 + rows, y_hi)
        try:
            # (median bar: a band at the rim of the lit region holds only pixels near FLOOR, where the 2^-36
            # accumulation quantum is up to TOL / 10 of the value; the sun's bands stay below 2e-6)
            rel, needed, c64 = _band_against_f64(pkg, lf, lens, W, H, y0, y1, spp, key, mask, min_lit=0,
                                                 median_bar=1e-5)
        except AssertionError:
            print(f"band {y0}..{y1} FAILED", flush=True)
            raise
        tot["bands"] += 1
        tot["rays"] += c64["rays_launched"]; tot["fragile"] += c64["rays_fragile"]
        if rel.size:
            tot["lit_bands"] += 1
            tot["values"] += int(rel.size); tot["needed"] += int(needed)
            tot["max_rel"] = max(tot["max_rel"], float(rel.max())); meds.append(float(np.median(rel)))
        print(f"band {y0}..{y1}: {rel.size} lit values, max rel {rel.max() if rel.size else 0:.2e}, "
              f"allowance needed {needed}, {time.time() - t0:.0f} s", flush=True)
    tot["median_of_band_medians"] = float(np.median(meds)) if meds else None
    tot["seconds"] = time.time() - t0
    print("WHOLE FRAME:", json.dumps(tot), flush=True)
    if y_lo == 0 and y_hi == H:
        assert tot["values"] > 100000
