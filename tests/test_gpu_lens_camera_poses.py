"""The scene imaged through decentred and tilted lenses (lf_set_lens_camera_surfaces(LF_LENSCAM_SURFACES_POSED); k_scene_lens<..,
3>, primary_row_general's pose branch, the pose records of lf_upload_primary_table):

  1. a posed lens's frame = the composition of the device's OWN rays (lf_generate_lens_rays at lf_lens_camera_samples), to
     1e-9 with the counters: both modes, films, stacks, the bilinear stop, sampled lights, an odd frame;
  2. identities, bit for bit: all-zero poses = the sphere-as-biconic lens under ALL; lenses without poses under POSED = what they
     were; records set and cleared; the row deal;
  3. the frame against the float64 tracer that moves the surface (tests/pose_ref.py), the bar Q taken from the kernels that exist;
     and lf_pose_event chained on the host over the primary rows in table order against lf_generate_lens_rays;
  4. a known answer that moves: a posed doublet displaces a distant emitter's image by more than three pixels;
  5. the setting's routing, the refusals' texts, the calibrated exposure against the tracer.

Every test here but the host chain (which holds the host event and lf_generate_lens_rays, both older than the setting) needs
LF_LENSCAM_SURFACES_POSED and fails on a library without it."""
import math

import numpy as np
import pytest

from goldenlib import load_texels
from oracle import lfo
from test_geo_rays_vs_f64 import W_TOL
from test_gpu_lens_camera import KEY, LIGHTS, SPHERES, TRIS, compose, sample_order, setup_scene_frame, unit_lights
from test_gpu_lens_camera_surfaces import centroid, device_rays, own_frame
from lens_camera_surfaces_lib import lens_of
from lens_camera_poses_lib import (ALLOWANCE_CAP, C2W, H, MOVE_H, MOVE_MASK, MOVE_MIN_PX, MOVE_W, MOVE_XY, MOVE_SENSOR_W_MM, NS, ODD, ONES, POS, W,
                                   WPM, displacement_px, films, host_chain, moved_emitter, posed_lens, trace, tracer_frame, tracer_samples)

import pose_ref as pr

pytestmark = pytest.mark.gpu
LF_ERR_INVALID, LF_ERR_UNSUPPORTED = 1, 6
TOL = 1e-9                                 # the bar of test_lens_frame_equals_the_float32_oracle


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture()
def lf(pkg):
    ctx = pkg.LensFlare(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def pentagon():
    return load_texels("pentbig500_14.png")


def configure(pkg, lf, name, mask, what="bare", w=W, h=H, ns=NS, surfaces=None):
    lens = dict(posed_lens(name))
    if "films" in what:
        lens["coatings"] = films()
    if "stacks" in what:
        lens["coating_stacks"] = pkg.load_lens_file("dgauss11_multicoated.lens")["coating_stacks"]
    setup_scene_frame(pkg, lf, lens, mask, w, h, ns, C2W, POS)
    lf.set_mask_filter(pkg.MASK_BILINEAR if "bilinear" in what else pkg.MASK_NEAREST)
    lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_POSED if surfaces is None else surfaces)
    lf.set_lens_camera_aim(0.0)
    return lens


def render(pkg, lf, mode):
    lf.set_lens_camera(mode, WPM, 0.0)
    lf.reset_scene_counters()
    lf.render_scene_term()
    return lf.read_buffer(pkg.SCENE_BUFFER), lf.scene_counters(), lf.lens_camera()


# ---- 1. the frame is the composition of the device's own rays -------------------------------------------------------------
OWN_CASES = [("bare", 1), ("bare", 2), ("films", 1), ("stacks", 1), ("bilinear", 1), ("stacks-bilinear", 1), ("odd", 1), ("odd", 2)]


@pytest.mark.parametrize("what,mode", OWN_CASES, ids=[f"{w}-mode{m}" for w, m in OWN_CASES])
def test_frame_is_the_composition_of_the_devices_own_rays(pkg, lf, pentagon, what, mode):
    """Under POSED the frame of dgauss11_decentred.lens = sum_s exposure * weight_s * L(exit ray_s) / (ns + 1) with the exit rays
    and weights lf_generate_lens_rays gives at lf_lens_camera_samples (k_march_path_rays<.., true, true>: bit for bit the ray
    the scene kernel queues), exposure and entrance pupil as lens_camera() reports them, the scene oracle's radiance: 1e-9,
    the bar of test_lens_frame_equals_the_float32_oracle, and its counters.  One case per FILT x STACK variant of the SURF = 3
    kernels, both modes, and the odd frame (no multiple of the tile, unstratified samples)."""
    w, h, ns = ODD if what == "odd" else (W, H, NS)
    lens = configure(pkg, lf, "decentred", pentagon, what, w, h, ns)
    got, cnt, info = render(pkg, lf, mode)
    got = got.reshape(-1, 3)
    assert info["mode"] == mode and info["exposure"] > 0
    z_ep, _ = pkg.paraxial_entrance_pupil(lens)
    assert info["entrance_pupil_z_mm"] == z_ep                 # (the centred lens's: the convention of DESIGN.md section 4)
    want, left = own_frame(lf, lens, mode, w, h, ns, info)
    assert cnt["lens_samples"] == w * h * ns * (3 if mode == 2 else 1) and cnt["lens_left"] == left
    assert (want.max(axis=-1) > 0.02).mean() > 0.5             # not a dark frame
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-12)
    print(f"decentred {what} mode {mode}: {left} of {cnt['lens_samples']} samples leave the lens, largest deviation {err.max():.2e}")
    assert err.max() <= TOL, err.max()


def test_frame_with_sampled_lights_is_the_composition_of_the_devices_own_rays(pkg, lf, pentagon):
    """SOFT = true (k_scene_lens<true, .., 3>): test_gpu_lens_camera_surfaces' sampled-lights case on the posed lens -- the
    device's own exit rays to the float64 scene oracle with the counter the device draws that sample's light samples from.
    Bar and fragility rule: tests/test_gpu_sampled_lights.py."""
    import sampled_lights_cases as slc
    configure(pkg, lf, "decentred", pentagon)
    sun = unit_lights(LIGHTS)[0]
    rows = [[0.0] + sun[4:7] + sun[1:4] + [0.0] * 9,
            [3.0, 6.0, 6.0, 5.0, 0.0, 2.5, -5.0, 0.0, -1.0, 0.0, 1.0, 0.0, 0.2, 0.0, 0.3, 1.0]]
    lf.set_scene_lights(rows)
    lf.set_light_samples(3)
    lf.set_lens_camera(1, WPM, 0.0)
    lf.render_scene_term()
    got = lf.read_buffer(pkg.SCENE_BUFFER).reshape(-1, 3)
    info = lf.lens_camera()
    desc = lfo.scene_desc(SPHERES, TRIS, rows, 3, False, None)
    number = np.empty(NS, np.uint32)
    number[sample_order(NS)] = np.arange(1, NS + 1)          # march sample -> sample number
    ctr = np.stack([np.repeat(np.arange(W * H, dtype=np.uint32), NS), np.tile(number, W * H)], -1)
    _, smp = device_rays(lf, 1, W * H)
    alive = (smp[..., 6] > 0).reshape(-1)
    with np.errstate(invalid="ignore"):
        o, d = lfo.lens_exit_to_world(smp[..., 0:3], smp[..., 3:6], C2W, POS, WPM, info["entrance_pupil_z_mm"])
    rays = np.concatenate([o, d, np.full(o.shape[:-1] + (1,), 0.01), np.full(o.shape[:-1] + (1,), 100.0)], -1)
    L = np.zeros((W * H * NS, 3))
    out, frag = lfo.scene_rays(desc, rays.reshape(-1, 8)[alive], ctr[alive], KEY)
    L[alive] = out[:, 5:8]
    fr = np.zeros(W * H * NS, bool)
    fr[alive] = frag
    fragile = fr.reshape(W * H, NS).any(axis=1)
    wgt = smp[..., 6].astype(np.float64).reshape(-1) * info["exposure"]
    want = (L * wgt[:, None]).reshape(W * H, NS, 3).sum(axis=1) / (NS + 1)
    assert (want.max(axis=-1) > 0.02).mean() > 0.5 and fragile.sum() <= slc.PIXEL_CAP * W * H, fragile.sum()
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    err[got == want] = 0.0
    print(f"decentred sampled lights: {int(fragile.sum())} fragile pixels, largest deviation {err[~fragile].max():.3e}")
    assert err[~fragile].max() <= slc.TOL


# ---- 2. identities, bit for bit -------------------------------------------------------------------------------------------
def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]


@pytest.mark.parametrize("mode", [1, 2])
def test_all_zero_poses_render_the_sphere_as_biconic_lens(pkg, lf, pentagon, mode):
    """Every posed interface with a record of zeros (R = I, t = 0) under POSED -- k_scene_lens<.., 3>, every such row through
    pose_event -- against the same lens without pose records, those interfaces written as biconics {1/R, 0, 0}, under ALL --
    k_scene_lens<.., 2>, biconic_event: the same frame, counters and calibration, bit for bit"""
    configure(pkg, lf, "zero", pentagon)
    assert lf.lens_poses()["n_posed"] == 4
    zero = render(pkg, lf, mode)
    configure(pkg, lf, "zero-bic", pentagon, surfaces=pkg.LENSCAM_SURFACES_ALL)
    assert lf.lens_poses()["n_posed"] == 0 and lf.lens_biconics()["n_biconic"] == 4
    bic = render(pkg, lf, mode)
    assert zero[0].max() > 0.02 and same(zero, bic)


@pytest.mark.parametrize("name", ["plain", "asph", "anam"])
def test_a_lens_without_poses_renders_the_same_bits_under_posed(pkg, lf, pentagon, name):
    """dgauss11.lens, dgauss11_asph.lens and dgauss11_anamorphic.lens under POSED: the frame, the counters and the calibration
    of SPHERICAL / ALL bit for bit, from one launch of the scene kernel each -- and a context whose pose records were set,
    used and cleared again.  What is held is the frame's bits and the COUNT of scene-kernel launches: the library reports
    no kernel name or variant for the scene term, so that a lens without poses does not launch k_scene_lens<.., 3> (which
    would render the same bits) rests on lf_render_scene_term picking SURF from pose.n alone, never from the setting."""
    lens = lens_of(name)
    frames = []
    for how in ("before", "posed", "danced"):
        setup_scene_frame(pkg, lf, lens, pentagon, W, H, NS, C2W, POS)
        before = pkg.LENSCAM_SURFACES_SPHERICAL if name == "plain" else pkg.LENSCAM_SURFACES_ALL
        lf.set_lens_camera_surfaces(before if how == "before" else pkg.LENSCAM_SURFACES_POSED)
        if how == "danced":
            n = int(lens["n"])
            on = np.zeros(n, np.int32); on[[0, n - 1]] = 1
            lf.set_lens_poses(on, np.tile([0.1, -0.05, 0.0], (n, 1)) * on[:, None], np.tile([0.3, 0.2, 10.0], (n, 1)) * on[:, None])
            lf.set_lens_camera(1, WPM, 0.0)
            lf.render_scene_term()                              # (the pose table is built and used ...)
            lf.set_lens_poses(None)                             # (... and the lens is un-posed again)
            assert lf.lens_poses()["n_posed"] == 0
        lf.timing_enable(True)
        lf.timing_reset()
        frames.append(render(pkg, lf, 1) + (lf.timing_get("scene_term")[0],))
        lf.timing_enable(False)
    assert frames[0][0].max() > 0.02 and frames[0][3] == 1
    for k in (1, 2):
        assert same(frames[0], frames[k]) and frames[k][3] == 1, k


def test_the_row_deal(pkg, lf, pentagon):
    """rank 1 of 2 renders exactly its tile rows of the single-context frame"""
    configure(pkg, lf, "decentred", pentagon)
    whole = render(pkg, lf, 1)[0]
    lf.set_scene_term(np.zeros((H, W, 3)))
    lf.set_row_interleave(1, 2)
    lf.render_scene_term()
    part = lf.read_buffer(pkg.SCENE_BUFFER)
    lf.set_row_interleave(0, 1)
    own = (np.arange(H) // 8) % 2 == 1
    assert whole.max() > 0.02 and np.array_equal(part[own], whole[own]) and not part[~own].any()


# ---- 3. the frame against float64 -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_frames(pkg):
    """{(lens, filmed): (frame, lens_camera() info, the device's starts)} in mode 1 under a mask of ones: the yardstick's lens
    under the default setting and the posed lens under POSED, bare and filmed, all four rendered here, once, in a context of
    their own -- no case depends on which ran first"""
    ctx = pkg.LensFlare(0)
    out = {}
    try:
        for name in ("plain", "decentred"):
            for filmed in (False, True):
                lens = dict(posed_lens(name))
                if filmed:
                    lens["coatings"] = films()
                setup_scene_frame(pkg, ctx, lens, ONES, W, H, NS, C2W, POS)
                ctx.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_SPHERICAL if name == "plain" else pkg.LENSCAM_SURFACES_POSED)
                ctx.set_lens_camera(1, WPM, 0.0)
                ctx.render_scene_term()
                out[(name, filmed)] = (ctx.read_buffer(pkg.SCENE_BUFFER).reshape(-1, 3), ctx.lens_camera(),
                                       ctx.lens_camera_samples(np.arange(W * H)))
    finally:
        ctx.close()
    return out


def against_tracer(device_frames, name, filmed, mode, traced_as=None):
    """(device frame, tracer frame, allowance) of a case; traced_as: the lens the TRACER follows (the neighbour clause)"""
    got, info, starts = device_frames[(name, filmed)]
    want, allow = np.zeros_like(got), np.zeros_like(got)
    for lam in ((1,) if mode == 1 else (0, 1, 2)):
        t = trace(traced_as or name, lam, starts, "device")
        f, a = tracer_frame(traced_as or name, t, filmed, (W * H, NS), info["entrance_pupil_z_mm"], info["exposure"])
        if mode == 1:
            want, allow = f, a
        else:
            want[:, lam], allow[:, lam] = f[:, lam], a[:, lam]
    return got, want, allow


def yardstick_q(device_frames, filmed, mode):
    """Q: dgauss11.lens under the default setting -- the kernels that exist -- against the same tracer at the device's samples:
    the largest relative deviation of a lit value (want > 1e-3) outside the allowance"""
    got, want, allow = against_tracer(device_frames, "plain", filmed, mode)
    assert allow.sum() < ALLOWANCE_CAP * want.sum()
    lit = want > 1e-3
    return float(np.max(np.maximum(np.abs(got - want) - allow, 0.0)[lit] / want[lit])), int(lit.sum())


@pytest.mark.parametrize("filmed", [False, True], ids=["bare", "filmed"])
def test_frame_against_the_float64_tracer(device_frames, filmed):
    """The reference: pose_ref.trace_path(lens, lam, -1, -1, ...) -- the ray stays, the surface moves -- at the device's
    samples, a mask of ones, composed by compose.  A sample the tracer finds within 4 D n_ev of an aperture rim MEASURED IN
    THE SURFACE'S OWN FRAME, or at incidence cosine <= 0.05, is fragile (lens_camera_poses_lib.tracer_frame), all allowances
    together below 2 % of the frame.  The bar comes from code that exists: Q, the largest relative deviation of a lit value
    outside the allowance when dgauss11.lens under the default setting meets the same tracer the same way in this run,
    0 < Q <= 2e-3; every value of the posed frame within 4 Q + allowance.  And the comparison tells the poses: the device frame
    misses the tracer's frame of the lens with its poses cleared by more than ten times what it misses its own by.  Measured
    on an MI355X: Q = 1.13e-4; the worst deviation outside the allowance 1.04 Q bare and filmed; allowance 0.50 % of the frame;
    own miss 3e-7 of the sum, poses cleared 3.7e-2."""
    q, n_lit = yardstick_q(device_frames, filmed, 1)
    print(f"yardstick {'filmed' if filmed else 'bare'}: Q = {q:.3e} over {n_lit} lit values")
    assert 0.0 < q <= 2e-3, q
    got, want, allow = against_tracer(device_frames, "decentred", filmed, 1)
    share = allow.sum() / want.sum()
    assert share < ALLOWANCE_CAP, share
    assert (want.max(axis=-1) > 0.02).mean() > 0.5
    dev = np.abs(got - want)
    over = dev - allow
    lit = want > 1e-3
    ratio = float(np.max(np.maximum(over, 0.0)[lit] / want[lit]) / q)
    print(f"decentred {'filmed' if filmed else 'bare'}: allowance {share:.2e} of the frame, worst deviation outside it {ratio:.3f} of Q "
          f"(bar 4), median relative deviation {np.median(dev[lit] / want[lit]):.2e}")
    assert (dev <= 4.0 * q * np.abs(want) + allow).all(), float(np.max((over - 4.0 * q * np.abs(want))))
    _, other, _ = against_tracer(device_frames, "decentred", filmed, 1, traced_as="cleared")
    own_miss, other_miss = float(np.abs(got - want).sum() / want.sum()), float(np.abs(got - other).sum() / want.sum())
    print(f"  summed |device - tracer| / summed tracer: own {own_miss:.2e}, poses cleared {other_miss:.2e}")
    assert other_miss > 10.0 * own_miss


def test_the_host_event_chained_in_table_order_is_the_devices_ray(pkg, lf):
    """lf_pose_event on the HOST, chained over the primary rows in the table's order -- row e is interface n - 1 - e, with ITS
    pose record, reflect = false, sgn = -1, n_in behind and n_out in front of the interface, dzv from the vertex the ray comes
    from (lens_camera_poses_lib.host_chain; the start ray, the stop and the un-posed rows are the float64 tracer's steps) --
    against lf_generate_lens_rays on dgauss11_decentred.lens, three wavelengths, tests/asphere_ref.py's grid of 588 rays: the
    contract {exit point, front_zv + hz, K = d in air, alive}.  The bar is test_gpu_poses' for path rays: exit point and
    direction within 4 D n_ev, D the yardstick of the shipped lens's posed faces (test_biconics_cpu._D), fates equal, rays the
    float64 tracer finds within the bar of a rim or at incidence cosine <= 0.05 left out (at most 2 %).  The check tells the
    order: with row e taking the pose record of interface e (k and e swapped) the chain misses the device by more than the bar.
    Measured on an MI355X: 0.0041 - 0.0046 of the bar (1.86e-3) in table order, 52 bars with k for e."""
    import asphere_ref as ar
    import test_biconics_cpu as tb
    import test_poses_cpu as tp
    from test_aspheres_cpu import COS_MIN
    lens = posed_lens("decentred")
    n = int(lens["n"])
    D = max(tb._D(s) for s in tp._cases()[:4])
    bar = 4 * D * n
    xy, uv = ar.comparison_grid()
    setup_scene_frame(pkg, lf, lens, ONES, W, H, NS, C2W, POS)
    assert lf.lens_poses()["n_posed"] == 4
    for lam in range(3):
        got = lf.generate_lens_rays(lam, xy, uv)
        ref, cmin, rim, _, _ = pr.trace_path(lens, lam, -1, -1, xy, uv, ONES)
        keep = ~((rim <= bar) | (cmin <= COS_MIN))
        assert (~keep).sum() <= 0.02 * len(xy), int((~keep).sum())
        worst = {}
        for how, pose_row in (("table order", None), ("k for e", lambda e: e)):
            chain = host_chain(lens, lam, xy, uv, pose_row)
            live = keep & (got[:, 7] == 1) & (chain[:, 7] == 1)
            assert live.sum() >= 20, (lam, how, int(live.sum()))
            gd = got[live, 3:6] / np.linalg.norm(got[live, 3:6], axis=1)[:, None]
            worst[how] = max(float(np.max(np.abs(got[live, 0:3] - chain[live, 0:3]))), float(np.max(np.abs(gd - chain[live, 3:6]))))
            if pose_row is None:
                assert np.array_equal(got[keep, 7] == 1, chain[keep, 7] == 1), lam
        print(f"lambda {lam}: host chain in table order misses the device's ray by {worst['table order'] / bar:.4f} of the bar "
              f"({bar:.2e}), with k for e by {worst['k for e'] / bar:.1f}")
        assert worst["table order"] <= bar and worst["k for e"] > bar


# ---- 4. a known answer that moves -----------------------------------------------------------------------------------------
def test_a_posed_doublet_moves_a_distant_emitters_image(pkg, lf):
    """dgauss11.lens with its doublet (interfaces 2 - 4) decentred and tilted as a rigid group (pose_group), a small emissive
    sphere 50 m away along the direction into which the float64 tracer sends the POSED lens's chief ray of sensor point
    MOVE_XY: the centroid of the device's image lies at that sensor point.  The tolerance is the existing known answer's: the
    float64-composed frame (the tracer at the device's samples of the pixels around the point) has a centroid of its own --
    twice its offset from the prediction plus 0.1 pixel.  The centred lens images the same sphere where ITS chief ray says,
    at least three pixels away (tests/test_lens_camera_poses_cpu.py holds the float64 side): the two device centroids lie more
    than 3 px minus the tolerance apart.  A kernel that ignores the pose, takes another row's, or turns it the wrong way
    fails here.  The stop is half closed (MOVE_MASK): at full aperture the posed doublet's coma pulls the centroid 1.3 px off
    the chief ray.  Measured on an MI355X: predicted (32.000, 21.600), float64-composed and device centroid both (32.387,
    21.241), tolerance 0.874 px; the chief rays 4.64 px apart, the device centroids 5.10 px."""
    Wk, Hk, ns, wpm = MOVE_W, MOVE_H, 16, 0.001
    lens, plain = posed_lens("moved"), posed_lens("unmoved")
    eye, origin = np.eye(3).reshape(-1), [0.0, 0.0, 0.0]
    z_ep, _ = pkg.paraxial_entrance_pupil(lens)
    emitter, _ = moved_emitter(z_ep, wpm)
    apart, there = displacement_px(z_ep)
    assert apart >= MOVE_MIN_PX
    setup_scene_frame(pkg, lf, lens, MOVE_MASK, Wk, Hk, ns, eye, origin, spheres=emitter, tris=[], lights=[])
    lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_POSED)
    lf.set_lens_camera(1, wpm, 0.0)
    lf.render_scene_term()
    img = lf.read_buffer(pkg.SCENE_BUFFER)
    info = lf.lens_camera()
    assert info["entrance_pupil_z_mm"] == z_ep
    pitch = MOVE_SENSOR_W_MM / Wk
    pred = (0.5 * Wk - MOVE_XY[0] / pitch, 0.5 * Hk - MOVE_XY[1] / pitch)
    got = centroid(img)
    lit = img.sum(axis=-1) > 0.04 * img.sum(axis=-1).max()
    assert 4 <= lit.sum() <= 60, lit.sum()                      # a few pixels
    x0, y0 = int(pred[0]) - 8, int(pred[1]) - 8
    ys, xs = np.mgrid[y0:y0 + 17, x0:x0 + 17]
    assert lit[y0:y0 + 17, x0:x0 + 17].sum() == lit.sum()
    pix = (ys * Wk + xs).reshape(-1)
    s = lf.lens_camera_samples(pix)
    t = pr.trace_path(lens, 1, -1, -1, s[..., 0:2], s[..., 2:4], MOVE_MASK)
    with np.errstate(invalid="ignore"):
        f, _, _ = compose(lens, MOVE_MASK, Wk, Hk, ns, eye, origin, wpm, info["entrance_pupil_z_mm"], info["exposure"],
                          tracer_samples(t, False, (len(pix), ns)), 6, emitter, [], [])
    ref = np.zeros((Hk, Wk, 3))
    ref[ys.reshape(-1), xs.reshape(-1)] = f
    want = centroid(ref)
    tol = 2.0 * max(abs(want[0] - pred[0]), abs(want[1] - pred[1])) + 0.1
    print(f"posed doublet: chief ray predicts pixel {pred[0]:.3f}, {pred[1]:.3f}; float64-composed centroid {want[0]:.3f}, {want[1]:.3f}; "
          f"device {got[0]:.3f}, {got[1]:.3f}; tolerance {tol:.3f} px; {int(lit.sum())} lit pixels")
    assert abs(got[0] - pred[0]) <= tol and abs(got[1] - pred[1]) <= tol
    # the same emitter through the centred lens: where its own chief ray says, three pixels and more away
    setup_scene_frame(pkg, lf, plain, MOVE_MASK, Wk, Hk, ns, eye, origin, spheres=emitter, tris=[], lights=[])
    lf.set_lens_camera(1, wpm, 0.0)
    lf.render_scene_term()
    cen = centroid(lf.read_buffer(pkg.SCENE_BUFFER))
    moved = math.hypot(got[0] - cen[0], got[1] - cen[1])
    print(f"  centred lens: chief ray predicts pixel {0.5 * Wk - there[0] / pitch:.3f}, {0.5 * Hk - there[1] / pitch:.3f}, device "
          f"{cen[0]:.3f}, {cen[1]:.3f}; the float64 chief rays lie {apart:.2f} px apart, the device centroids {moved:.2f} px")
    assert moved > MOVE_MIN_PX - tol


# ---- 5. routing, refusals, exposure ---------------------------------------------------------------------------------------
def test_setting_routing_and_refusals(pkg, lf, pentagon):
    lens = posed_lens("decentred")
    setup_scene_frame(pkg, lf, lens, pentagon, W, H, NS, C2W, POS)
    assert pkg.LENSCAM_SURFACES_POSED == 3 and lf.lens_camera_surfaces() == pkg.LENSCAM_SURFACES_SPHERICAL
    lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_POSED)
    assert lf.lens_camera_surfaces() == 3
    for bad in (2, -1):
        with pytest.raises(pkg.LensFlareError) as e:
            lf.set_lens_camera_surfaces(bad)
        assert e.value.status == LF_ERR_INVALID
    assert lf.lens_camera_surfaces() == 3                        # (a refused value changes nothing)
    lf.set_lens_camera(1, WPM, 0.0)
    # a posed lens under 0 and under 1: refused, by both calls, with a text that names both setters
    for which in (pkg.LENSCAM_SURFACES_SPHERICAL, pkg.LENSCAM_SURFACES_ALL):
        lf.set_lens_camera_surfaces(which)
        for call in (lf.render_scene_term, lf.lens_camera):
            with pytest.raises(pkg.LensFlareError) as e:
                call()
            assert e.value.status == LF_ERR_UNSUPPORTED
            assert "lf_set_lens_poses" in str(e.value) and "lf_set_lens_camera_surfaces" in str(e.value)
    # under 3 both accept it
    lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_POSED)
    assert math.isfinite(lf.lens_camera()["exposure"])
    lf.render_scene_term()
    assert lf.read_buffer(pkg.SCENE_BUFFER).max() > 0.02
    # the per-lane kernel has no instantiation for poses
    try:
        lf.test_knob("scene_compact", 0)
        with pytest.raises(pkg.LensFlareError) as e:
            lf.render_scene_term()
        assert e.value.status == LF_ERR_UNSUPPORTED and "scene_compact" in str(e.value)
    finally:
        lf.test_knob("scene_compact", -1)


@pytest.mark.parametrize("mask_name", ["pentagon", "smooth"])
def test_calibrated_exposure_against_the_tracer(pkg, lf, pentagon, mask_name):
    """lens_camera() under POSED on the posed lens: 4096 / the float64 tracer's summed on-axis weights over the 64 x 64 cell
    centres of the pupil square, within W_TOL (calibrate_exposure goes through lf_generate_lens_rays, which follows the poses)"""
    mask = pentagon if mask_name == "pentagon" else np.random.default_rng(20261019).uniform(0.25, 1.0, (16, 16)).astype(np.float32)
    lens = posed_lens("decentred")
    setup_scene_frame(pkg, lf, lens, mask, W, H, NS, C2W, POS)
    lf.set_lens_camera_surfaces(pkg.LENSCAM_SURFACES_POSED)
    lf.set_lens_camera(1, WPM, 0.0)
    got = lf.lens_camera()["exposure"]
    g = (np.float32(2.0) * (np.arange(64, dtype=np.float32) + np.float32(0.5))) / np.float32(64.0) - np.float32(1.0)
    uv = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)
    t = pr.trace_path(lens, 1, -1, -1, np.zeros_like(uv), uv, mask)
    want = 4096.0 / t[0][:, 6].sum()
    print(f"exposure decentred {mask_name}: device {got:.9g}, tracer {want:.9g}, relative {abs(got / want - 1.0):.2e}")
    assert math.isfinite(got) and abs(got - want) <= W_TOL * want
