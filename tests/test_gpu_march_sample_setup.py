"""The culled march's per-sample set-up and the admission to its weighted re-march (lens-flare_amd/csrc/lf_cull.hip,
lf_march_common.h lobe_gate, lf_march.hip):

  * a listed sample carries the pupil sub-cell its listing pass drew (k_march_cull's s_list: the sample's place in the
    chunk and both sub-cell indices in one LDS dword), so the wave that marches it does not draw again;
  * the lanes admitted by the loose pre-test d.s > lobe_thr are narrowed by the epilogue's own test lobe_q < 1 on the first
    march's direction BEFORE the weighted re-march, and a wavelength none of whose lanes passes is not marched again.

Neither may move a pixel or a counted event; only the two re-march tallies may fall.  On the frame of
tests/test_gpu_march_moves.py (1920 x 1080, the bench's mask and c3's sun, cull_force, the tile rows through the sun's row)
every case holds

  * the culled launch (mode 2) to the full enumeration (mode 0): the ghost buffer bit for bit, rays_hit_light, and the
    fates summing to the rays launched;
  * the culled launch to every started path marched alone (cull_no_prefix: march_started_path, MODE 0 of the kernel):
    pixels, every counter, both re-march tallies;
  * the audit to lit == 0 and the launch's reason to "applied".

The cases are the smallest at which each new branch can go wrong: 16 samples (G = 4, every sample stratified and drawn)
with 6, 2 and 0 sub-cell bits (0: the item kernel, whose lanes draw nothing but pass the gate); 20 samples (4 unstratified
ones take the block's union entry and carry no draw); 1 sample; tile strides 1 and 8; eight wavelengths (groups of
3 + 3 + 2); a 640-pixel frame (blocks smaller than the wave tile: every lane looks its own row up, the draw is still the
wave's); and whole 1280 x 720 frames, where the launch's last tiles are split over several workgroups that read the listed
draws through their own sample stride -- at 4 samples (the launch does not split a tile below 32 samples per workgroup, so
this one runs the unsplit path on a whole frame) and at 64 (two workgroups per tail tile).

The gate: on the two-row band with all pairs the tallies are positive and not above the parent commit's for the same launch
(constants below), and the float32 oracle's frame and counters are the launch's, as in test_gpu_march_moves.py."""
import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo

pytestmark = pytest.mark.gpu
RAD = [1.0, 0.9, 0.5]
SUN_NS = (0.521445, 0.517156)     # bench.py: where the c3 frame's sun lands
KEY = 0x1e45f1a4e
ONE_ROW, TWO_ROWS = (552, 560), (552, 568)

# the parent commit's re-march tallies (b890a3f, its library on an MI355X) for the launch of test_gate_*: 1920 x 1080,
# rows 552..568, 16 samples, all pairs and the primary path, culling mode 2
PARENT_REMARCH_ROWS = 222705
PARENT_REMARCH_LANE_EVENTS = 10300577


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="module")
def lf(pkg):
    ctx = pkg.LensFlare(0)
    lfo.geo_follow_device(ctx)
    ctx.test_knob("cull_force", 1)
    yield ctx
    ctx.test_knob("cull_force", 0)
    lfo.geo_follow_device(None)
    ctx.close()


@pytest.fixture(scope="module")
def mask():
    return load_texels("pentbig500_14.png")


def _sun(pkg, lens, W, H):
    efl, sw = pkg.paraxial_efl(lens), lens["sensor_width_mm"]
    return [(SUN_NS[0] - 0.5) * sw / efl, (SUN_NS[1] - 0.5) * sw * H / W / efl, -1.0]


def _setup(pkg, lf, lens, mask, W, H, band, lambda_rgb=None):
    lf.set_frame(W, H)
    lf.set_mask_filter(pkg.MASK_NEAREST)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    if lambda_rgb is not None:
        lf.set_lambda_rgb(lambda_rgb)
    lf.set_sun(_sun(pkg, lens, W, H), RAD, 0.05)
    lf.set_ghost_pairs(None, True)
    if band is not None:
        lf.set_band(*band)
    lf.set_row_interleave(0, 1)


def _launch(pkg, lf, spp, mode, no_prefix=False):
    lf.set_march_culling(mode)
    lf.test_knob("cull_no_prefix", 1 if no_prefix else 0)
    try:
        lf.reset_counters()
        lf.trace_ghosts(spp, KEY)
        return dict(ghost=lf.read_buffer(pkg.GHOST_BUFFER).copy(), counters=lf.counters(), stats=lf.march_stats(),
                    executed=lf.executed_events(), culled=lf.cull_info()["culled"], reason=lf.cull_reason(),
                    audit=lf.cull_audit(), table=lf.cull_table_and_block())
    finally:
        lf.test_knob("cull_no_prefix", 0)


def _restore(pkg, lf):
    lf.set_mask_filter(pkg.MASK_NEAREST)
    lf.set_pupil_subcells(pkg.DEFAULT_SUBCELL_BITS)
    lfo.lib().geo_set_sub_bits(pkg.DEFAULT_SUBCELL_BITS)
    lf.set_tile_stride(pkg.DEFAULT_TILE_STRIDE)
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(1)
    lf.set_frame(64, 64)                  # (the whole frame is the band again)


def _device_legs(pkg, lf, W, H, band, spp, n_lambda, n_paths=46, rows_by_wave_order=False):
    """the culled launch, the same with every started path alone, the full enumeration: what must hold between them
    (rows_by_wave_order: the item kernel fills its waves in the order its LDS atomics arrive, and a wavelength is marched
    again for a whole wave -- its re-march ROWS differ from launch to launch of the same frame, its lane events do not)"""
    y0, y1 = band if band is not None else (0, H)
    culled = _launch(pkg, lf, spp, 2)
    alone = _launch(pkg, lf, spp, 2, no_prefix=True)
    full = _launch(pkg, lf, spp, 0)
    assert culled["culled"] and alone["culled"] and not full["culled"]
    assert culled["reason"] == "applied" and alone["reason"] == "applied"
    assert culled["audit"]["rays"] > 0 and culled["audit"]["lit"] == 0
    assert full["ghost"][y0:y1].max() > 0 and not full["ghost"][:y0].any() and not full["ghost"][y1:].any()
    assert np.array_equal(culled["ghost"], full["ghost"])
    c1, c0 = culled["counters"], full["counters"]
    assert c0["rays_launched"] == W * (y1 - y0) * spp * n_lambda * n_paths
    assert 0 < c1["rays_launched"] <= c0["rays_launched"]
    assert c1["rays_hit_light"] == c0["rays_hit_light"] > 0
    assert c1["rays_launched"] == c1["rays_clipped_stop"] + c1["rays_vignetted"] + c1["rays_tir"] + c1["rays_reached_scene"]
    assert c0["rays_launched"] == c0["rays_clipped_stop"] + c0["rays_vignetted"] + c0["rays_tir"] + c0["rays_reached_scene"]
    # every started path alone: the same frame, every counter, both re-march tallies
    assert np.array_equal(alone["ghost"], culled["ghost"]) and alone["counters"] == c1
    for k in ("remarch_lane_events", "remarch_rows"):
        assert alone["stats"][k] > 0 and culled["stats"][k] > 0, k
        if k == "remarch_lane_events" or not rows_by_wave_order:
            assert alone["stats"][k] == culled["stats"][k], k
    assert alone["executed"] == c1["surface_events"]
    assert 0 < culled["executed"] <= c1["surface_events"]
    print("started", c1["rays_launched"], "of", c0["rays_launched"], "rays; lit", c1["rays_hit_light"], "re-march rows",
          culled["stats"]["remarch_rows"], "lane events", culled["stats"]["remarch_lane_events"], "(full enumeration:",
          full["stats"]["remarch_rows"], full["stats"]["remarch_lane_events"], ")")
    return culled, full


BAND_CASES = {
    # name: (lens file, W, H, band, samples, sub-cell bits, tile stride)
    "bits2": ("dgauss11.lens", 1920, 1080, ONE_ROW, 16, 2, None),
    "bits0_item_kernel": ("dgauss11.lens", 1920, 1080, ONE_ROW, 16, 0, None),
    "unstratified_tail_of_20": ("dgauss11.lens", 1920, 1080, ONE_ROW, 20, None, None),
    "one_sample": ("dgauss11.lens", 1920, 1080, TWO_ROWS, 1, None, None),
    "stride1": ("dgauss11.lens", 1920, 1080, ONE_ROW, 16, None, 1),
    "stride8": ("dgauss11.lens", 1920, 1080, ONE_ROW, 16, None, 8),
    "eight_wavelengths": ("dgauss11_8lambda.lens", 1920, 1080, ONE_ROW, 16, None, None),
    "rows_per_lane_640": ("dgauss11.lens", 640, 360, (176, 192), 16, None, None),     # 32-pixel blocks under a 64-pixel wave tile
    "whole_frame_4": ("dgauss11.lens", 1280, 720, None, 4, None, None),
    "whole_frame_64_split_tail": ("dgauss11.lens", 1280, 720, None, 64, None, None),
}


@pytest.mark.parametrize("name", list(BAND_CASES))
def test_culled_is_the_full_enumeration(pkg, lf, mask, name):
    lens_name, W, H, band, spp, bits, stride = BAND_CASES[name]
    lens = pkg.load_lens_file(lens_name)
    n_lambda = int(np.asarray(lens["ior"]).shape[0])
    lam = pkg.spectral_weights(lens["lambda_nm"])[0] if n_lambda != 3 else None
    try:
        _setup(pkg, lf, lens, mask, W, H, band, lambda_rgb=lam)
        if bits is not None:
            lf.set_pupil_subcells(bits)
        if stride is not None:
            lf.set_tile_stride(stride)
        culled, _ = _device_legs(pkg, lf, W, H, band, spp, n_lambda, rows_by_wave_order=(bits == 0))
        if name == "rows_per_lane_640":
            assert culled["table"][1] < 64       # the blocks ARE smaller than the wave tile
    finally:
        _restore(pkg, lf)


def test_gate_tallies_fall_and_the_oracle_holds(pkg, lf, mask):
    """the default sampling (6 sub-cell bits) on the two-row band with all pairs: the re-march tallies against the parent
    commit's, the frame and every counter against the float32 oracle under the device's own table"""
    W, H, spp = 1920, 1080, 16
    lens = pkg.load_lens_file("dgauss11.lens")
    y0, y1 = TWO_ROWS
    try:
        _setup(pkg, lf, lens, mask, W, H, TWO_ROWS)
        culled, full = _device_legs(pkg, lf, W, H, TWO_ROWS, spp, 3)
        rows, lanes = culled["stats"]["remarch_rows"], culled["stats"]["remarch_lane_events"]
        print("re-march rows", rows, "parent", PARENT_REMARCH_ROWS, "lane events", lanes, "parent", PARENT_REMARCH_LANE_EVENTS)
        assert 0 < rows <= PARENT_REMARCH_ROWS
        assert 0 < lanes <= PARENT_REMARCH_LANE_EVENTS
        # (the path tree passes the same gate: the same tallies of the paths it completes inside the pre-test)
        assert 0 < full["stats"]["remarch_rows"] and 0 < full["stats"]["remarch_lane_events"]
        og, oc = lfo.geo_trace(lens, W, H, y0, y1, spp, KEY, None, True, mask, _sun(pkg, lens, W, H), RAD, 0.05,
                               n_threads=16, cull=culled["table"])
        assert lfo.last_culled_lit == 0
        assert (og > 0).any() and np.array_equal(culled["ghost"], og)
        assert oc == culled["counters"], (oc, culled["counters"])
    finally:
        _restore(pkg, lf)
