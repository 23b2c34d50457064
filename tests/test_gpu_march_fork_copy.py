"""The shared-leg march after its fork was turned round (lens-flare_amd/csrc/lf_cull.hip march_started_set: the common leg
stays in its registers and a started path runs its own rows on a COPY taken at the fork, so nothing is taken back;
started_row is the one row body of both loops) and its lit epilogue trimmed (lf_march_common.h lobe_gate hands the
epilogue the q it computed on the first march's direction; the three channel factors are read off one address; the
re-march tallies are summed per sample in 32 bits).  Nothing the kernels compute may move.  On the frame of
tests/test_gpu_march_moves.py (1920 wide, the bench's mask and sun, 16 samples so that G = 4, culling forced, the one or
two 8-row tile rows through the sun's row) every case compares the culled launch

  * with the full enumeration (the path tree, culling off): the ghost buffer bit for bit;
  * with every started path marched alone (lf_test_knob cull_no_prefix: march_started_path, which copies nothing and
    whose epilogue is its own): the same pixels, every counter and both re-march tallies, and no more rows executed than
    counted;
  * with the float32 oracle under the device's own table: pixels and every march counter bit for bit, and the oracle
    finds no lit ray in what the table dropped.

The cases are the smallest that reach each changed line: all 45 pairs and the primary path on two tile rows (legs extended
by every length, a leg that dies before the next fork); (2,4)+(2,7), where the second path forks where the first did (the
leg is extended by zero rows and the first own row's sequence dword comes from the load before the leg loop);
(1,4)+(6,9); (2,7) alone; the primary path alone (no fork: the copy is taken at the leg's end); (2,7) and the primary
path; eight wavelengths (groups of 3 + 3 + 2: a group whose third state does not exist).  A coated lens and the bilinear
mask -- which the oracle follows neither of -- are held to the full enumeration and to every path alone, and so is a
context of two lights, whose kVarLights kernel runs the new fork in front of its unchanged epilogue (lights_epilogue).

The oracle alone, on the CPU, says every band holds light (tests/test_gpu_march_moves.py records the lit pixels: 22025 /
449+ / 1108 / 2168 / 10995); each test asserts (og > 0).any() again."""
import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo

pytestmark = pytest.mark.gpu
RAD = [1.0, 0.9, 0.5]
RAD2 = [0.5, 1.0, 0.8]
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
    lf.set_ghost_pairs(None, True)
    lf.set_march_culling(1)
    lf.set_frame(64, 64)                  # (the whole frame is the band again)


def _device_legs(pkg, lf, band, n_paths, n_lambda):
    """the culled launch against the full enumeration and against every started path alone"""
    y0, y1 = band
    culled = _launch(pkg, lf, 2)
    alone = _launch(pkg, lf, 2, no_prefix=True)
    full = _launch(pkg, lf, 0)
    assert culled["culled"] and alone["culled"] and not full["culled"]
    assert culled["audit"]["rays"] > 0 and culled["audit"]["lit"] == 0
    # ---- the full enumeration: the ghost buffer bit for bit
    assert full["ghost"][y0:y1].max() > 0 and not full["ghost"][:y0].any() and not full["ghost"][y1:].any()
    assert np.array_equal(culled["ghost"], full["ghost"])
    c1, c0 = culled["counters"], full["counters"]
    assert c0["rays_launched"] == W * (y1 - y0) * SPP * n_lambda * n_paths
    assert 0 < c1["rays_launched"] <= c0["rays_launched"]                 # a path was started
    assert c1["rays_hit_light"] == c0["rays_hit_light"] > 0
    assert c1["rays_launched"] == c1["rays_clipped_stop"] + c1["rays_vignetted"] + c1["rays_tir"] + c1["rays_reached_scene"]
    # ---- every started path alone: pixels, every counter, both re-march tallies; the shared leg only executes fewer rows
    assert np.array_equal(alone["ghost"], culled["ghost"])
    assert alone["counters"] == c1, (alone["counters"], c1)
    for k in ("remarch_lane_events", "remarch_rows"):
        assert alone["stats"][k] == culled["stats"][k] > 0, k
    assert alone["executed"] == c1["surface_events"]
    assert 0 < culled["executed"] <= c1["surface_events"]
    return culled, full


BARE_CASES = {
    # name: (lens file, pairs, primary, band, paths)
    "all_pairs_and_primary": ("dgauss11.lens", None, True, TWO_ROWS, 46),
    "two_pairs_same_first_mirror": ("dgauss11.lens", [(2, 4), (2, 7)], False, ONE_ROW, 2),       # the leg extended by zero rows
    "two_pairs_other_first_mirrors": ("dgauss11.lens", [(1, 4), (6, 9)], False, ONE_ROW, 2),
    "one_pair": ("dgauss11.lens", [(2, 7)], False, ONE_ROW, 1),
    "primary_alone": ("dgauss11.lens", [(-1, -1)], False, ONE_ROW, 1),                           # no fork: the copy at the leg's end
    "one_pair_and_primary": ("dgauss11.lens", [(2, 7)], True, ONE_ROW, 2),
    "eight_wavelengths": ("dgauss11_8lambda.lens", None, True, ONE_ROW, 46),                     # groups of 3 + 3 + 2
}


@pytest.mark.parametrize("name", list(BARE_CASES))
def test_fork_on_a_copy_is_the_full_enumeration_every_path_alone_and_the_oracle(pkg, lf, mask, name):
    lens_name, pairs, primary, band, n_paths = BARE_CASES[name]
    lens = pkg.load_lens_file(lens_name)
    n_lambda = int(np.asarray(lens["ior"]).shape[0])
    lam = pkg.spectral_weights(lens["lambda_nm"])[0] if n_lambda != 3 else None
    try:
        _setup(pkg, lf, lens, mask, band, pairs, primary, lambda_rgb=lam)
        culled, full = _device_legs(pkg, lf, band, n_paths, n_lambda)
        # ---- the oracle under the device's table: pixels and all counters bit for bit
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


@pytest.mark.parametrize("lens_name,bilinear", [("dgauss11_coated.lens", False), ("dgauss11.lens", True)])
def test_film_and_bilinear_kernels_fork_on_a_copy(pkg, lf, mask, lens_name, bilinear):
    """the kVarCoat and kVarFilt instantiations of the shared-leg kernel, which the oracle does not follow: held to the full
    enumeration (the path tree keeps its own loops) and to every started path alone"""
    lens = pkg.load_lens_file(lens_name)
    filt = pkg.MASK_BILINEAR if bilinear else pkg.MASK_NEAREST
    try:
        _setup(pkg, lf, lens, mask, TWO_ROWS, filt=filt)
        assert lf.lens_coatings()["n_coated"] == (8 if "coated" in lens_name else 0)
        culled, _ = _device_legs(pkg, lf, TWO_ROWS, 46, 3)
        # the bare, nearest frame differs: the variant's code ran
        _setup(pkg, lf, pkg.load_lens_file("dgauss11.lens"), mask, TWO_ROWS)
        plain = _launch(pkg, lf, 2)
        assert not np.array_equal(plain["ghost"], culled["ghost"])
    finally:
        _restore(pkg, lf)


def test_two_lights_fork_on_a_copy_in_front_of_the_unchanged_epilogue(pkg, lf, mask):
    """lf_set_lights with two lights: the kVarLights kernel runs the new fork, lights_pretest on the copy and its own
    lights_epilogue -- the culled frame is the full enumeration's and that of every started path alone"""
    lens = pkg.load_lens_file("dgauss11.lens")
    sun = _sun(pkg, lens)
    second = [sun[0] + 0.004, sun[1], -1.0]          # its lobe overlaps the sun's: some rays lie in both
    try:
        _setup(pkg, lf, lens, mask, TWO_ROWS)
        one = _launch(pkg, lf, 2)
        lf.set_lights([sun, second], [RAD, RAD2], [0.05, 0.03])
        assert len(lf.lights()[2]) == 2
        culled, full = _device_legs(pkg, lf, TWO_ROWS, 46, 3)
        # the second light is seen: more (ray, light) contributions than the sun's alone, and another frame
        assert culled["counters"]["rays_hit_light"] > one["counters"]["rays_hit_light"] > 0
        assert not np.array_equal(culled["ghost"], one["ghost"])
    finally:
        lf.set_sun(sun, RAD, 0.05)
        _restore(pkg, lf)
