"""The tracer's side of tests/test_gpu_lens_camera_poses.py, no device needed: random starts over the sensor and the pupil
square, 24 576 rays (the GPU frame's count), a mask of ones.

  * the fragile samples' allowance (rim distance in the surface's own frame) stays below the cap the GPU test holds it to;
  * the poses matter to a frame: the tracer-composed frame of the posed lens differs from that of the lens with its poses cleared;
  * pose_ref.trace_path on the primary path with all-zero poses is biconic_ref's on the same lens, to 1e-12;
  * the known answer moves: the posed doublet displaces a distant emitter's image by at least three pixels;
and, host only, the new constant and the ABI."""
import os
import re

import numpy as np

import biconic_ref as br
import pose_ref as pr
from lens_camera_poses_lib import (ALLOWANCE_CAP, H, MOVE_MIN_PX, MOVE_XY, NS, ONES, W, displacement_px, films, fragile, package, posed_lens,
                                   pose_D, random_starts, trace, tracer_frame)

STARTS = random_starts(20261021)
SHAPE = (W * H, NS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def z_ref(name):
    return package().paraxial_entrance_pupil(posed_lens(name))[0]


def test_the_constant_and_the_abi():
    pkg = package()
    assert pkg.LENSCAM_SURFACES_POSED == 3 and (pkg.LENSCAM_SURFACES_SPHERICAL, pkg.LENSCAM_SURFACES_ALL) == (0, 1)
    header = open(os.path.join(ROOT, "include", "lensflare.h")).read()
    assert re.search(r"LF_LENSCAM_SURFACES_POSED\s*=\s*3\b", header)
    lib = pkg.load_library()
    for sym in ("lf_set_lens_camera_surfaces", "lf_get_lens_camera_surfaces", "lf_set_lens_poses"):
        assert sym in pkg.ABI_SYMBOLS and hasattr(lib, sym), sym
    # without a context the value 3 is refused like any value (no symbol is missing)
    for which in (0, 1, 2, 3):
        assert lib.lf_set_lens_camera_surfaces(None, which) == 1          # LF_ERR_INVALID


def test_the_fragile_allowance_stays_under_its_cap():
    """dgauss11_decentred.lens: the allowance the GPU test composes -- a fragile sample's weight times the radiance its own ray
    finds -- bare and filmed, below 2 % of the frame; the rim distance is that of the hit in the surface's frame"""
    t = trace("decentred", 1, STARTS, "random")
    n_fragile = int(fragile("decentred", t).sum())
    for filmed in (False, True):
        want, allow = tracer_frame("decentred", t, filmed, SHAPE, z_ref("decentred"), 1.0)
        share = float(allow.sum() / want.sum())
        print(f"decentred {'filmed' if filmed else 'bare'}: {n_fragile} fragile samples (D = {pose_D():.3e}), allowance {share:.2e} of "
              f"the frame; smallest incidence cosine {t[1].min():.3f}")
        assert (want.max(axis=-1) > 0).mean() > 0.5 and 0.0 < share < ALLOWANCE_CAP


def test_the_poses_matter_to_the_frame():
    t, t0 = trace("decentred", 1, STARTS, "random"), trace("cleared", 1, STARTS, "random")
    with_rec, _ = tracer_frame("decentred", t, False, SHAPE, z_ref("decentred"), 1.0)
    without, _ = tracer_frame("cleared", t0, False, SHAPE, z_ref("decentred"), 1.0)
    miss = float(np.abs(with_rec - without).sum() / with_rec.sum())
    print(f"the frame with its poses cleared differs by {miss:.3e} of the summed value")
    assert miss > 1e-3


def test_all_zero_poses_trace_as_the_biconic_tracer():
    """pose_ref moves the surface, biconic_ref knows none: with every decentre and angle zero both trace the same primary
    path on the same lens -- exit point, direction, weights, the smallest cosine and rim -- to 1e-12"""
    s = STARTS.reshape(-1, 4)[::16]
    a = pr.trace_path(posed_lens("zero"), 1, -1, -1, s[:, 0:2], s[:, 2:4], ONES, films())
    b = br.trace_path(posed_lens("cleared"), 1, -1, -1, s[:, 0:2], s[:, 2:4], ONES, films())
    alive = b[0][:, 7] == 1.0
    assert np.array_equal(a[0][:, 7], b[0][:, 7]) and 0.2 < alive.mean() < 0.9
    assert np.abs(a[0][alive] - b[0][alive]).max() <= 1e-12
    assert np.abs(a[4] - b[4]).max() <= 1e-12 and np.array_equal(a[3], b[3])
    assert np.abs(a[1] - b[1])[alive].max() <= 1e-12 and np.abs(a[2] - b[2])[alive].max() <= 1e-12


def test_the_posed_doublet_moves_the_image_by_three_pixels():
    """The known answer of the GPU test: the emitter lies on the posed lens's chief ray of MOVE_XY; the centred lens's chief
    ray through the same emitter starts at another sensor point, at least three pixels of the frame away"""
    pkg = package()
    z_ep = pkg.paraxial_entrance_pupil(posed_lens("moved"))[0]
    assert z_ep == pkg.paraxial_entrance_pupil(posed_lens("unmoved"))[0]          # (everything paraxial is the centred lens's)
    px, there = displacement_px(z_ep)
    print(f"posed sensor point {MOVE_XY}, centred {there[0]:.4f}, {there[1]:.4f} mm: {px:.2f} px apart")
    assert px >= MOVE_MIN_PX
