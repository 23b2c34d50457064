"""The tracer's side of tests/test_gpu_lens_camera_surfaces.py, no device needed: random starts over the sensor and the pupil
square, 24 576 rays (the GPU frame's count), a mask of ones.

  * the fragile samples' allowance stays below the cap the GPU test holds it to, for both recorded lenses;
  * the records matter to a frame: the tracer-composed frame of each recorded lens differs from that of the lens with its
    records dropped by more than 1e-3 of the summed value -- which makes the GPU test's neighbour clause meaningful;
  * the Python tracer's primary path is anchored to the float64 tracer under oracle/: on dgauss11.lens both compose the same
    frame within the existing float64 frame bars.
And, host only, the new ABI's declarations."""
import numpy as np
import pytest

from oracle import lfo
from lens_camera_surfaces_lib import (ALLOWANCE_CAP, C2W, H, NS, ONES, POS, W, WPM, crude_allowance, lens_of, package, random_starts,
                                      trace, tracer_frame, tracer_samples)
from test_gpu_lens_camera import LIGHTS, SPHERES, TRIS, compose

STARTS = random_starts(20261020)
SHAPE = (W * H, NS)


def z_ref(name):
    return package().paraxial_entrance_pupil(lens_of(name))[0]


@pytest.mark.parametrize("name", ["asph", "anam"])
def test_the_fragile_allowance_stays_under_its_cap(name):
    """the crude bound -- fragile count x largest weight / summed weight -- and the allowance the GPU test composes (weight
    times the radiance the sample's own ray finds), bare and filmed: both below 2 % of the frame"""
    t = trace(name, 1, STARTS, "random")
    for filmed in (False, True):
        crude = crude_allowance(name, t, filmed)
        want, allow = tracer_frame(name, t, filmed, SHAPE, z_ref(name), 1.0)
        share = float(allow.sum() / want.sum())
        print(f"{name} {'filmed' if filmed else 'bare'}: crude bound {crude:.2e}, composed allowance {share:.2e} of the frame; "
              f"smallest incidence cosine {t[1].min():.3f}")
        assert 0.0 < crude < ALLOWANCE_CAP and share < ALLOWANCE_CAP


@pytest.mark.parametrize("name", ["asph", "anam"])
def test_the_records_matter_to_the_frame(name):
    t, t0 = trace(name, 1, STARTS, "random"), trace(name + "-dropped", 1, STARTS, "random")
    for filmed in (False, True):
        with_rec, _ = tracer_frame(name, t, filmed, SHAPE, z_ref(name), 1.0)
        without, _ = tracer_frame(name + "-dropped", t0, filmed, SHAPE, z_ref(name), 1.0)
        miss = float(np.abs(with_rec - without).sum() / with_rec.sum())
        print(f"{name} {'filmed' if filmed else 'bare'}: the frame with its records dropped differs by {miss:.3e} of the summed value")
        assert miss > 1e-3


def test_the_python_tracer_composes_the_frame_of_the_float64_oracle():
    """asphere_ref's primary path (through biconic_ref.trace_path, which calls its events) against lfo.g64_lens_rays at the same
    starts on dgauss11.lens: the bars of test_lens_frame_against_the_independent_float64_tracer -- 2e-3 (+ allowance) on every
    value, 1e-4 (+ allowance) on more than 99.5 % -- the allowance the summed potential weight of the samples either tracer
    calls fragile"""
    lens = lens_of("plain")
    z, e = z_ref("plain"), lfo.lens_exposure(lens, W, ONES)
    t = trace("plain", 1, STARTS, "random")
    ours, allow = tracer_frame("plain", t, False, SHAPE, z, e)
    g = lfo.g64_lens_rays(lens, 1, STARTS[..., 0:2], STARTS[..., 2:4], ONES).reshape(SHAPE + (10,))
    theirs, L, _ = compose(lens, ONES, W, H, NS, C2W, POS, WPM, z, e, g, 6, SPHERES, TRIS, LIGHTS)
    allow = allow + ((g[..., 8] > 0) * g[..., 7] * e * L.max() / (NS + 1)).sum(axis=1)[:, None]
    alive_ours, alive_theirs = tracer_samples(t, False, SHAPE)[..., 6] > 0, g[..., 6] > 0
    print(f"alive: {int(alive_ours.sum())} / {int(alive_theirs.sum())} of {alive_ours.size}, fates differ on "
          f"{int((alive_ours != alive_theirs).sum())}; allowance {allow.sum() / theirs.sum():.2e} of the frame")
    dev = np.abs(ours - theirs)
    lit = theirs > 1e-3
    print(f"largest relative deviation of a lit value {np.max(dev[lit] / theirs[lit]):.3e}, median {np.median(dev[lit] / theirs[lit]):.3e}")
    assert (theirs.max(axis=-1) > 0.02).mean() > 0.5
    assert (dev <= 2e-3 * np.abs(theirs) + allow + 1e-13).all()
    assert (dev <= 1e-4 * np.abs(theirs) + allow + 1e-13).mean() > 0.995


def test_the_abi_declares_the_setting_and_the_samples_call():
    pkg = package()
    lib = pkg.load_library()
    for sym in ("lf_set_lens_camera_surfaces", "lf_get_lens_camera_surfaces", "lf_lens_camera_samples"):
        assert sym in pkg.ABI_SYMBOLS and hasattr(lib, sym), sym
    assert (pkg.LENSCAM_SURFACES_SPHERICAL, pkg.LENSCAM_SURFACES_ALL) == (0, 1)
    for call in (lib.lf_set_lens_camera_surfaces(None, 1), lib.lf_get_lens_camera_surfaces(None, None),
                 lib.lf_lens_camera_samples(None, 0, None, None)):
        assert call == 1          # LF_ERR_INVALID without a context
