"""The culled march after its register moves were taken out of the row loops (lens-flare_amd/csrc/lf_march_common.h
weighted_remarch: the weight record read as the single dwords one wavelength needs, the sequence dword one row ahead;
lf_cull.hip: the per-channel factor of a lit ray formed once per workgroup).  Nothing the kernels compute may move: on
the bench's frame (1920 wide, the bench's mask and sun, 16 samples so that G = 4, culling mode 2: the shared-leg kernel)
the one or two 8-row tile rows through the sun's row are compared

  * with the full enumeration (the path tree, culling off), bit for bit;
  * with the float32 oracle under the device's own table, bit for bit, pixels and every march counter;
  * with every started path marched alone (lf_test_knob cull_no_prefix: march_started_path through the same
    weighted_remarch): the same pixels, counters and re-march tallies, and as many rows executed as counted.

The cases are the smallest that reach each changed line: all 45 pairs and the primary path; pair subsets that fork at
the same and at different first mirrors, one pair (no take-back), the primary path (no fork), one pair and the primary
path; eight wavelengths (groups of 3 + 3 + 2: the last group's third wavelength does not exist); a coated lens (the
record's film offset through the narrow load), the bilinear mask, and both: the four variants of the kernels; and the
independent-pixel specification, whose item kernel calls the same re-march.

The oracle follows neither a film nor the bilinear lookup (tests/test_gpu_coatings.py, test_gpu_mask_filter.py): those
variants are held to the full enumeration -- whose kernel keeps its own weighted loop, untouched here -- bit for bit, and
a coated frame's counters to the oracle's of the bare lens (a film never touches geometry).

The oracle alone, on the CPU, says every band below holds light (lit pixels: all pairs 22025 on two tile rows; on one:
(2,4)+(2,7) and (2,7) alone 449+, (1,4)+(6,9) 1108, primary 2168, eight wavelengths 10995); each test asserts it again."""
import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo

pytestmark = pytest.mark.gpu
RAD = [1.0, 0.9, 0.5]
SUN_NS = (0.521445, 0.517156)     # bench.py: where the c3 frame's sun lands (row 558 of 1080: tile row 69)
W, H, SPP, KEY = 1920, 1080, 16, 0x1e45f1a4e
ONE_ROW, TWO_ROWS = (552, 560), (552, 568)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="module")
def lf(pkg):
    ctx = pkg.LensFlare(0)
    lfo.geo_follow_device(ctx)
    # (16 samples make the table's cells coarse: it starts more than the launch would keep the culled kernel for)
    ctx.test_knob("cull_force", 1)
    yield ctx
    ctx.test_knob("cull_force", 0)
    lfo.geo_follow_device(None)
    ctx.close()


@pytest.fixture(scope="module")
def mask():
    return load_texels("pentbig500_14.png")


def _sun(pkg, lens):
    efl, sw = pkg.paraxial_efl(lens), lens["sensor_width_mm"]
    return [(SUN_NS[0] - 0.5) * sw / efl, (SUN_NS[1] - 0.5) * sw * H / W / efl, -1.0]


def _setup(pkg, lf, lens, mask, band, pairs=None, primary=True, lambda_rgb=None, filt=None):
    lf.set_frame(W, H)
    lf.set_mask_filter(pkg.MASK_NEAREST if filt is None else filt)
    lf.set_aperture(pkg.APERTURE_STARBURST, mask)
    lf.set_lens(lens)
    if lambda_rgb is not None:
        lf.set_lambda_rgb(lambda_rgb)
    lf.set_sun(_sun(pkg, lens), RAD, 0.05)
    lf.set_ghost_pairs(pairs, primary)
    lf.set_band(*band)
    lf.set_row_interleave(0, 1)


def _launch(pkg, lf, mode, no_prefix=False):
    lf.set_march_culling(mode)
    lf.test_knob("cull_no_prefix", 1 if no_prefix else 0)
    try:
        lf.reset_counters()
        lf.trace_ghosts(SPP, KEY)
        return dict(ghost=lf.read_buffer(pkg.GHOST_BUFFER).copy(), counters=lf.counters(), stats=lf.march_stats(),
                    executed=lf.executed_events(), culled=lf.cull_info()["culled"], audit=lf.cull_audit(),
                    table=lf.cull_table_and_block())
    finally:
        lf.test_knob("cull_no_prefix", 0)


def _restore(pkg, lf):
    lf.set_mask_filter(pkg.MASK_NEAREST)
    lf.set_pupil_subcells(pkg.DEFAULT_SUBCELL_BITS)
    lfo.lib().geo_set_sub_bits(pkg.DEFAULT_SUBCELL_BITS)
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(1)
    lf.set_frame(64, 64)                  # (the whole frame is the band again)


def _device_legs(pkg, lf, band, n_paths, n_lambda):
    """the culled launch, the same with every started path alone, the full enumeration: what must hold between them"""
    y0, y1 = band
    culled = _launch(pkg, lf, 2)
    alone = _launch(pkg, lf, 2, no_prefix=True)
    full = _launch(pkg, lf, 0)
    assert culled["culled"] and alone["culled"] and not full["culled"]
    assert culled["audit"]["rays"] > 0 and culled["audit"]["lit"] == 0
    assert full["ghost"][y0:y1].max() > 0 and not full["ghost"][:y0].any() and not full["ghost"][y1:].any()
    assert np.array_equal(culled["ghost"], full["ghost"])
    c1, c0 = culled["counters"], full["counters"]
    assert c0["rays_launched"] == W * (y1 - y0) * SPP * n_lambda * n_paths
    assert 0 < c1["rays_launched"] <= c0["rays_launched"]                 # a path was started
    assert c1["rays_hit_light"] == c0["rays_hit_light"] > 0
    assert c1["rays_launched"] == c1["rays_clipped_stop"] + c1["rays_vignetted"] + c1["rays_tir"] + c1["rays_reached_scene"]
    # every started path alone: the same frame, counters and re-march tallies; the shared leg only executes fewer rows
    assert np.array_equal(alone["ghost"], culled["ghost"]) and alone["counters"] == c1
    for k in ("remarch_lane_events", "remarch_rows"):
        assert alone["stats"][k] == culled["stats"][k] > 0, k
    assert alone["executed"] == c1["surface_events"]
    assert 0 < culled["executed"] <= c1["surface_events"]
    return culled, full


BARE_CASES = {
    # name: (lens file, pairs, primary, band, paths)
    "all_pairs_and_primary": ("dgauss11.lens", None, True, TWO_ROWS, 46),
    "two_pairs_same_first_mirror": ("dgauss11.lens", [(2, 4), (2, 7)], False, ONE_ROW, 2),       # the second forks where the first did
    "two_pairs_other_first_mirrors": ("dgauss11.lens", [(1, 4), (6, 9)], False, ONE_ROW, 2),
    "one_pair": ("dgauss11.lens", [(2, 7)], False, ONE_ROW, 1),                                  # the group's last path: no take-back
    "primary_alone": ("dgauss11.lens", [(-1, -1)], False, ONE_ROW, 1),                           # no fork
    "one_pair_and_primary": ("dgauss11.lens", [(2, 7)], True, ONE_ROW, 2),
    "eight_wavelengths": ("dgauss11_8lambda.lens", None, True, ONE_ROW, 46),                     # groups of 3 + 3 + 2
}


@pytest.mark.parametrize("name", list(BARE_CASES))
def test_band_is_the_full_enumeration_and_the_oracle(pkg, lf, mask, name):
    lens_name, pairs, primary, band, n_paths = BARE_CASES[name]
    lens = pkg.load_lens_file(lens_name)
    n_lambda = int(np.asarray(lens["ior"]).shape[0])
    lam = pkg.spectral_weights(lens["lambda_nm"])[0] if n_lambda != 3 else None
    try:
        _setup(pkg, lf, lens, mask, band, pairs, primary, lambda_rgb=lam)
        culled, full = _device_legs(pkg, lf, band, n_paths, n_lambda)
        y0, y1 = band
        og, oc = lfo.geo_trace(lens, W, H, y0, y1, SPP, KEY, pairs, primary, mask, _sun(pkg, lens), RAD, 0.05,
                               n_threads=16, lambda_rgb=lam, cull=culled["table"])
        assert lfo.last_culled_lit == 0
        assert (og > 0).any() and np.array_equal(culled["ghost"], og)
        assert oc == culled["counters"], (oc, culled["counters"])
        print(name, "lit pixels", int((og > 0).any(axis=2).sum()), "started", culled["counters"]["rays_launched"], "of",
              full["counters"]["rays_launched"], "rays; rows executed", culled["executed"], "counted",
              culled["counters"]["surface_events"], "re-march rows", culled["stats"]["remarch_rows"])
    finally:
        _restore(pkg, lf)


@pytest.mark.parametrize("lens_name,bilinear", [("dgauss11_coated.lens", False), ("dgauss11.lens", True),
                                                ("dgauss11_coated.lens", True)])
def test_film_and_bilinear_variants(pkg, lf, mask, lens_name, bilinear):
    lens = pkg.load_lens_file(lens_name)
    filt = pkg.MASK_BILINEAR if bilinear else pkg.MASK_NEAREST
    band = TWO_ROWS
    try:
        _setup(pkg, lf, lens, mask, band, filt=filt)
        assert lf.lens_coatings()["n_coated"] == (8 if "coated" in lens_name else 0)
        culled, full = _device_legs(pkg, lf, band, 46, 3)
        # the bare, nearest frame differs (the variant's code ran) ...
        bare = pkg.load_lens_file("dgauss11.lens")
        _setup(pkg, lf, bare, mask, band)
        plain = _launch(pkg, lf, 2)
        assert not np.array_equal(plain["ghost"], culled["ghost"])
        if not bilinear:
            # ... but a film never touches geometry: the table and the counters are the bare lens', which the oracle follows
            assert np.array_equal(plain["table"][0], culled["table"][0])
            assert plain["counters"] == culled["counters"] and plain["stats"] == culled["stats"]
            _, oc = lfo.geo_trace(bare, W, H, band[0], band[1], SPP, KEY, None, True, mask, _sun(pkg, bare), RAD, 0.05,
                                  n_threads=16, cull=culled["table"])
            assert lfo.last_culled_lit == 0 and oc == culled["counters"]
        # the independent-pixel specification: the item kernel's re-march of the same variant, against the path tree
        _setup(pkg, lf, lens, mask, ONE_ROW, filt=filt)
        lf.set_pupil_subcells(0)
        items, tree = _launch(pkg, lf, 2), _launch(pkg, lf, 0)
        assert items["culled"] and not tree["culled"] and items["audit"]["lit"] == 0
        assert tree["ghost"].max() > 0 and np.array_equal(items["ghost"], tree["ghost"])
        assert items["counters"]["rays_hit_light"] == tree["counters"]["rays_hit_light"] > 0
        assert items["stats"]["remarch_rows"] > 0
    finally:
        _restore(pkg, lf)


@pytest.mark.parametrize("lens_name", ["dgauss11.lens", "dgauss11_8lambda.lens"])
def test_independent_pixels_through_the_item_kernel(pkg, lf, mask, lens_name):
    """lf_set_pupil_subcells(0): k_march_items lists (pixel, sample) items by path and marches them through
    march_started_path -- the same weighted_remarch -- against the path tree and the oracle"""
    lens = pkg.load_lens_file(lens_name)
    n_lambda = int(np.asarray(lens["ior"]).shape[0])
    lam = pkg.spectral_weights(lens["lambda_nm"])[0] if n_lambda != 3 else None
    y0, y1 = ONE_ROW
    try:
        _setup(pkg, lf, lens, mask, ONE_ROW, lambda_rgb=lam)
        lf.set_pupil_subcells(0)
        lfo.lib().geo_set_sub_bits(0)
        items, tree = _launch(pkg, lf, 2), _launch(pkg, lf, 0)
        assert items["culled"] and not tree["culled"] and items["audit"]["lit"] == 0
        assert np.array_equal(items["ghost"], tree["ghost"])
        assert items["counters"]["rays_hit_light"] == tree["counters"]["rays_hit_light"] > 0
        assert items["stats"]["remarch_rows"] > 0 and items["executed"] == items["counters"]["surface_events"]
        og, oc = lfo.geo_trace(lens, W, H, y0, y1, SPP, KEY, None, True, mask, _sun(pkg, lens), RAD, 0.05,
                               n_threads=16, lambda_rgb=lam, cull=items["table"])
        assert lfo.last_culled_lit == 0
        assert (og > 0).any() and np.array_equal(items["ghost"], og) and oc == items["counters"]
    finally:
        _restore(pkg, lf)
