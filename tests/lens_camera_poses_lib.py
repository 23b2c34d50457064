"""What tests/test_gpu_lens_camera_poses.py and tests/test_lens_camera_poses_cpu.py share: the posed lenses, the float64 tracer
of tests/pose_ref.py on the primary path at given starts (cached: a trace of 24 576 rays takes seconds), the fragile-sample rule
with the rim measured in the surface's own frame, the composition of a tracer frame with its allowance, and the known answer
that moves (a posed doublet displaces a distant emitter's image).  Not a test module."""
import numpy as np

import pose_ref as pr
from lens_camera_surfaces_lib import ALLOWANCE_CAP, C2W, H, NS, ODD, ONES, POS, W, WPM, package, random_starts, tracer_samples, yardstick_D  # noqa: F401
from test_aspheres_cpu import COS_MIN
from test_gpu_lens_camera import LIGHTS, SPHERES, TRIS, compose

# the known answer: dgauss11.lens, its cemented doublet (interfaces 2 - 4) decentred and tilted about its front vertex as a
# rigid group (pose_group), on a sensor narrow enough that the displacement of the image is several pixels of a 96-pixel row
MOVE_FIRST, MOVE_LAST = 2, 4
MOVE_DECENTRE, MOVE_TILT = (0.6, -0.4, 0.0), (1.0, -0.8, 0.0)
MOVE_SENSOR_W_MM, MOVE_W, MOVE_H = 6.0, 96, 64
MOVE_XY = (1.0, 0.65)                      # the sensor point whose chief ray aims the emitter (mm)
MOVE_MIN_PX = 3.0
# (the stop half closed -- the central 2 x 2 of 4 x 4 texels: the posed doublet's coma, which pulls a full-aperture centroid off
# the chief ray by more than a pixel and would widen the measured tolerance with it, goes with the square of the aperture)
MOVE_MASK = np.zeros((4, 4), np.float32)
MOVE_MASK[1:3, 1:3] = 1.0

_cache = {}


def posed_lens(name):
    """'decentred': dgauss11_decentred.lens (a rotated toroid on interface 1, the doublet 2 - 4 decentred and tilted);
    'cleared': the same prescription without its pose records (it keeps the toroid's biconic record);
    'zero': the same interfaces posed, every decentre and angle zero;
    'zero-bic': no pose record, every interface 'zero' poses written as a biconic (a sphere: Rx = R, kx = ky = 0);
    'plain': dgauss11.lens;  'moved' / 'unmoved': the known answer's lens with and without its pose records"""
    if name in _cache:
        return _cache[name]
    pkg = package()
    if name == "plain":
        lens = pkg.load_lens_file("dgauss11.lens")
    elif name in ("moved", "unmoved"):
        lens = dict(pkg.load_lens_file("dgauss11.lens"), sensor_width_mm=MOVE_SENSOR_W_MM)
        if name == "moved":
            pivot = float(np.sum(np.asarray(lens["thickness"], np.float64)[:MOVE_FIRST]))
            lens["poses"] = pkg.pose_group(lens, MOVE_FIRST, MOVE_LAST, pivot, MOVE_DECENTRE, MOVE_TILT)
    else:
        lens = dict(pkg.load_lens_file("dgauss11_decentred.lens"))
        po = lens["poses"]
        if name == "cleared":
            del lens["poses"]
        elif name == "zero":
            lens["poses"] = dict(on=po["on"].copy(), decentre=np.zeros_like(po["decentre"]), tilt_deg=np.zeros_like(po["tilt_deg"]))
        elif name == "zero-bic":
            del lens["poses"]
            b = {k: np.array(v) for k, v in lens["biconics"].items()}
            for k in np.flatnonzero(po["on"]):
                if not b["on"][k]:
                    b["on"][k] = 1
                    b["radius_x"][k] = lens["radius"][k]
            lens["biconics"] = b
        elif name != "decentred":
            raise KeyError(name)
    _cache[name] = lens
    return lens


def films():
    """dgauss11_coated.lens's films: every lens here has the double Gauss's eleven interfaces"""
    return package().load_lens_file("dgauss11_coated.lens")["coatings"]


def trace(name, lam, starts, tag):
    """pose_ref.trace_path on the primary path at starts (n, 4) {X, Y, pa, pb} under a mask of ones, traced ONCE per (lens,
    wavelength, tag) with the films: the filmed weight in column 6 of [0], the bare lens's weight in [4]"""
    key = ("trace", name, lam, tag)
    if key not in _cache:
        s = np.asarray(starts, np.float32).reshape(-1, 4)
        _cache[key] = pr.trace_path(posed_lens(name), lam, -1, -1, s[:, 0:2], s[:, 2:4], ONES, films())
    return _cache[key]


def pose_D():
    """the event yardstick D: a posed face runs the biconic event (a sphere as a biconic) -- yardstick_D of the biconic route"""
    return yardstick_D("anam")


def fragile(name, t):
    """a sample is fragile where the tracer met an aperture rim within 4 D n_ev or an incidence cosine of 0.05 or less.  The rim
    distance of a posed interface is pose_ref.event's: |sqrt(q_x^2 + q_y^2) - h| of the hit q in the SURFACE's frame"""
    n_ev = int(posed_lens(name)["n"])
    return (t[2] <= 4 * pose_D() * n_ev) | (t[1] <= COS_MIN)


def tracer_frame(name, t, filmed, shape, z_ref, exposure, pose=(C2W, POS, WPM), scene=(SPHERES, TRIS, LIGHTS)):
    """lens_camera_surfaces_lib.tracer_frame with this module's lenses and fragile rule: (frame, allowance), each (n_pix, 3).
    A fragile sample the tracer passed may add or remove its weight times the radiance its ray finds; one the tracer killed
    and marched on gets the frame's largest weight times the radiance its ray finds; one that went on nowhere gets none."""
    n_pix, ns = shape
    lens = posed_lens(name)
    smp = tracer_samples(t, filmed, shape)
    c2w, pos, wpm = pose
    with np.errstate(invalid="ignore"):
        want, L, alive = compose(lens, ONES, 0, 0, ns, c2w, pos, wpm, z_ref, exposure, smp, 6, *scene)
        fr = fragile(name, t).reshape(shape)
        w = smp[..., 6]
        went_on = np.isfinite(smp[..., 0:6]).all(axis=-1)
        pot = smp.copy()
        pot[..., 6] = np.where(fr & alive, w, np.where(fr & ~alive & went_on, w.max(), 0.0))
        pot[..., 0:6] = np.where((pot[..., 6] > 0)[..., None], pot[..., 0:6], [0.0, 0.0, 0.0, 0.0, 0.0, -1.0])
        allow = compose(lens, ONES, 0, 0, ns, c2w, pos, wpm, z_ref, exposure, pot, 6, *scene)[0]
    return want, allow


# ---- the host event chained over the primary rows ------------------------------------------------------------------------------
def host_chain(lens, lam, sensor_xy, pupil_uv, pose_row=None):
    """The primary path in the TABLE's order -- row e = 0 .. n - 1 is interface k = n - 1 - e -- with every posed row marched by
    the library's HOST event (lf_pose_event, float32) under the arguments the primary table gives a row: reflect = false,
    sgn = -1 (forward = 0), n_in the medium behind the interface, n_out the one in front, dzv = the vertex the ray comes from
    minus this one, K = n_in d.  The start ray, the stop and the un-posed rows are pose_ref.trace_path's own float64 steps.
    pose_row(e) names the interface whose pose record row e takes (None: its own, n - 1 - e).  Returns (n x 8 as trace_path's
    [0], without a weight; fates alive / dead in column 7)."""
    import asphere_ref as ar
    import biconic_ref as br
    pkg = package()
    G = pr.lens_geometry(lens)
    n = G["n"]
    xy = np.asarray(sensor_xy, np.float32).astype(np.float64).reshape(-1, 2)
    uv = np.asarray(pupil_uv, np.float32).astype(np.float64).reshape(-1, 2)
    qx, qy = ar.pupil_disc(uv[:, 0], uv[:, 1])
    hp, vz = G["h"][-1], G["zv"][-1] - G["z_sensor"]
    p = np.stack([xy[:, 0], xy[:, 1], np.full(len(xy), G["z_sensor"])], axis=1)
    v = np.stack([hp * qx - xy[:, 0], hp * qy - xy[:, 1], np.full(len(xy), vz)], axis=1)
    d = v / np.linalg.norm(v, axis=1)[:, None]
    alive = np.ones(len(xy), bool)
    ior = G["ior"][lam]
    for e in range(n):
        k = n - 1 - e
        if k == G["stop"]:
            t = (G["zv"][k] - p[:, 2]) / d[:, 2]
            p = p + t[:, None] * d
            alive &= p[:, 0] ** 2 + p[:, 1] ** 2 <= G["h"][k] ** 2
            continue
        n_before = 1.0 if k == 0 else ior[k - 1] if k - 1 != G["stop"] else (1.0 if k - 2 < 0 else ior[k - 2])
        n_in, n_out = ior[k], n_before                     # the ray travels -z: from behind the interface to in front of it
        if G["pose_on"][k]:
            kp = k if pose_row is None else pose_row(e)
            z_from = G["z_sensor"] if k == n - 1 else G["zv"][k + 1]
            rays = np.concatenate([p[:, 0:2], (p[:, 2] - z_from)[:, None], n_in * d], axis=1).astype(np.float32)
            cx = G["cx"][k] if G["bic_on"][k] else G["c"][k]
            out, fates = pkg.pose_event(cx, G["c"][k], G["kx"][k], G["ky"][k], None, G["pose_t"][kp], G["pose_a"][kp], G["h"][k],
                                        n_in, n_out, 0, 0, np.float32(z_from - G["zv"][k]), rays)
            out = out.astype(np.float64)
            p = np.stack([out[:, 0], out[:, 1], G["zv"][k] + out[:, 2]], axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                d = out[:, 3:6] / np.linalg.norm(out[:, 3:6], axis=1)[:, None]
            alive &= fates == 0
        else:
            if G["bic_on"][k]:
                ev = br.event(p, d, G["zv"][k], G["cx"][k], G["c"][k], G["kx"][k], G["ky"][k], G["h"][k], n_in, n_out, False, None)
            else:
                ev = ar.event(p, d, G["zv"][k], G["c"][k], G["kappa"][k], G["coef"][:, k], G["h"][k], n_in, n_out, False, None)
            p, d = ev["p"], ev["d"]
            alive &= ev["fate"] == pr.ALIVE
    out = np.zeros((len(xy), 8))
    out[:, 0:3] = p; out[:, 3:6] = d; out[:, 7] = alive
    return out


# ---- the known answer that moves --------------------------------------------------------------------------------------------
def chief_ray(name, xy):
    """the tracer's exit ray of pupil point (0, 0) of sensor point xy at the middle wavelength: n x 8"""
    out = pr.trace_path(posed_lens(name), 1, -1, -1, np.atleast_2d(xy), np.zeros((len(np.atleast_2d(xy)), 2)), ONES)[0]
    assert (out[:, 7] == 1.0).all()
    return out


def moved_emitter(z_ep, wpm=0.001, dist=50.0, radius=0.1):
    """(emitter sphere, its centre in lens millimetres): 50 m along the posed lens's chief ray of MOVE_XY, the camera's pose the
    identity at the origin"""
    c = chief_ray("moved", MOVE_XY)[0]
    o = np.array([c[0], c[1], c[2] - z_ep]) * wpm
    d = c[3:6] / np.linalg.norm(c[3:6])
    centre = o + dist * d
    return [tuple(centre) + (radius, "e", 5.0, 5.0, 5.0)], centre / wpm + np.array([0.0, 0.0, z_ep])


def sensor_point_of(name, target_mm, start_xy):
    """the sensor point of lens `name` whose float64 chief ray passes through target_mm (lens coordinates): Newton on the
    chief ray's miss in the plane through the target across the axis, central differences"""
    xy = np.array(start_xy, np.float64)

    def miss(p):
        c = chief_ray(name, p)[0]
        s = (target_mm[2] - c[2]) / c[5]
        return (c[0:3] + s * c[3:6])[0:2] - target_mm[0:2]
    for _ in range(6):
        m, h = miss(xy), 1e-3
        J = np.stack([(miss(xy + [h, 0.0]) - miss(xy - [h, 0.0])) / (2 * h), (miss(xy + [0.0, h]) - miss(xy - [0.0, h])) / (2 * h)], axis=1)
        xy = xy - np.linalg.solve(J, m)
    assert np.abs(miss(xy)).max() < 1.0    # mm at 50 m: 2e-5 rad, a hundredth of a pixel on the sensor
    return xy


def displacement_px(z_ep):
    """how far, in pixels of the known answer's frame, the posed lens's image of the emitter lies from the centred lens's:
    the float64 chief rays of both"""
    _, target = moved_emitter(z_ep)
    there = sensor_point_of("unmoved", target, MOVE_XY)
    pitch = MOVE_SENSOR_W_MM / MOVE_W
    return float(np.linalg.norm(there - np.array(MOVE_XY)) / pitch), there
