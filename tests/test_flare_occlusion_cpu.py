"""Flare occlusion without a device (lf_set_flare_occlusion): the five prototypes are declared, exported and wrapped, the
setter refuses what the contract refuses (the wrapper before anything reaches the library; the library itself is asked on
the device, tests/test_gpu_flare_occlusion.py), lf_flare_shadow_samples is the stated low-discrepancy set, and
lf_flare_shadow_rays is the float64 restatement below BIT FOR BIT.

The restatements here (samples64, rays64, shadow_ray64, quad_margin) are what the GPU tests count with as well."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lens-flare_amd", "host")
CTX_SYMBOLS = ["lf_set_flare_occlusion", "lf_get_flare_occlusion", "lf_get_flare_visibility"]
HOST_SYMBOLS = ["lf_flare_shadow_samples", "lf_flare_shadow_rays"]
CAMERA, FRONT = 0, 1
FLARES = [(0.5, 0.5), (0.7, 0.6), (0.2, 0.35)]
HFOV, VFOV, ALPHA, WPM = 40.0, 27.0, 0.00465, 0.001
PI_ = 3.14159265358979323      # (the literal of find_sun_pos' kernel)


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


# ---- the float64 restatements -------------------------------------------------------------------------------------------
def radical_inverse(r, base):
    v, f = 0.0, 1.0 / base
    while r:
        v += f * (r % base)
        r //= base
        f /= base
    return v


def samples64(R):
    """the contract's samples in float64 (libm's sin and cos), R x 4: a b c d"""
    out = np.zeros((R, 4), np.float64)
    for r in range(R):
        u0, u1, u2, u3 = (r + 0.5) / R, radical_inverse(r, 2), radical_inverse(r, 3), radical_inverse(r, 5)
        out[r] = (np.sqrt(u0) * np.cos(2 * np.pi * u1), np.sqrt(u0) * np.sin(2 * np.pi * u1),
                  np.sqrt(u2) * np.cos(2 * np.pi * u3), np.sqrt(u2) * np.sin(2 * np.pi * u3))
    return out


def flare_dir64(flare, hfov=HFOV, vfov=VFOV):
    """s = unit((2 nx - 1) edge_x, (2 ny - 1) edge_y, -1) and e1, e2, each operation the contract's, in its order"""
    nx, ny = np.float64(flare[0]), np.float64(flare[1])
    edge_x = np.float64(np.tan(0.5 * (hfov * (PI_ / 180.0))))
    edge_y = np.float64(np.tan(0.5 * (vfov * (PI_ / 180.0))))
    vx, vy, vz = (2.0 * nx - 1.0) * edge_x, (2.0 * ny - 1.0) * edge_y, np.float64(-1.0)
    vn = np.sqrt((vx * vx + vy * vy) + vz * vz)
    s = np.array([vx / vn, vy / vn, vz / vn])
    ux, uy, uz = s[2], np.float64(0.0), -s[0]
    un = np.sqrt((ux * ux + uy * uy) + uz * uz)
    e1 = np.array([ux / un, uy / un, uz / un])
    e2 = np.array([s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]])
    return s, e1, e2


def rays64(samples32, flare, alpha, origin, h0, hfov=HFOV, vfov=VFOV):
    """lf_flare_shadow_rays restated in numpy float64 on the library's own float32 sample table, narrowed to float32"""
    t = np.asarray(samples32, np.float32).astype(np.float64)
    s, e1, e2 = flare_dir64(flare, hfov, vfov)
    ta = np.float64(np.tan(np.float64(np.float32(alpha))))
    out = np.zeros((len(t), 6), np.float32)
    for k in range(3):
        out[:, 3 + k] = (s[k] + ta * (t[:, 2] * e1[k] + t[:, 3] * e2[k])).astype(np.float32)
    if origin == FRONT:
        h = np.float64(np.float32(h0))
        out[:, 0] = (h * t[:, 0]).astype(np.float32)
        out[:, 1] = (h * t[:, 1]).astype(np.float32)
    return out


def shadow_ray64(rays32, wpm, z_ref, x_flip=1.0, use_z_ref=True, wpm_power=1):
    """the ghost march's shadow-ray mapping for the identity pose at the origin: world origin and unit direction, float64.
    The keyword arguments are the mutants a wrong mapping would be."""
    r = np.asarray(rays32, np.float32).astype(np.float64)
    w = wpm ** wpm_power
    o = np.stack([x_flip * r[:, 0] * w, r[:, 1] * w, (r[:, 2] - (z_ref if use_z_ref else 0.0)) * w], 1)
    d = r[:, 3:]
    rn = 1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = d * rn[:, None]
    d[:, 0] *= x_flip
    return o, d


def quad_margin(o, d, z_plane, x0, x1, y0, y1):
    """rays against the axis-aligned quad [x0, x1] x [y0, y1] in the plane z = z_plane: (hit, margin) -- margin = the
    distance, in world units, of the ray's point in the plane from the quad's nearest edge line, and (in barycentric terms
    times the shorter side) from the diagonal its two triangles share: how far the ray is from flipping"""
    t = (z_plane - o[:, 2]) / d[:, 2]
    x, y = o[:, 0] + t * d[:, 0], o[:, 1] + t * d[:, 1]
    hit = (t > 0.0) & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    diag = np.abs((x - x0) / (x1 - x0) - (y - y0) / (y1 - y0)) * min(x1 - x0, y1 - y0)
    margin = np.min(np.abs(np.stack([x - x0, x - x1, y - y0, y - y1, diag], 1)), axis=1)
    return hit, margin


def beam_centre_x(flare, z_plane, origin, wpm, z_ref):
    """where the flare's beam centre -- the ray of the sample (0, 0, 0, 0) -- meets the plane z = z_plane"""
    s, _, _ = flare_dir64(flare)
    oz = -z_ref * wpm if origin == FRONT else 0.0
    return float(s[0] * ((z_plane - oz) / s[2]))


# ---- the tests ------------------------------------------------------------------------------------------------------
def test_the_five_prototypes_are_declared_exported_and_wrapped():
    pkg = _pkg()
    header = open(os.path.join(ROOT, "include", "lensflare.h")).read()
    lib = pkg.load_library()
    for s in CTX_SYMBOLS:
        assert re.search(r"lf_status\s+%s\s*\(\s*lf_ctx\s*\*" % s, header), s
        assert s in pkg.ABI_SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s)(*([C.c_void_p(0)] * 6)) == 1, s      # a NULL context: LF_ERR_INVALID, nothing dereferenced
    assert re.search(r"^lf_status\s+lf_flare_shadow_samples\s*\(\s*int rays_per_light,\s*float\s*\*\s*out\)", header, re.M)
    assert re.search(r"^lf_status\s+lf_flare_shadow_rays\s*\(\s*int rays_per_light,\s*const double flare_origin\[2\],\s*double hfov_deg,\s*"
                     r"double vfov_deg,\s*float angular_radius,\s*int origin,\s*float front_semi_aperture,\s*float\s*\*\s*rays\)", header, re.M)
    for s in HOST_SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.lf_flare_shadow_samples(C.c_int(64), C.c_void_p(0)) == 1
    assert "typedef enum { LF_FLARE_ORIGIN_CAMERA = 0, LF_FLARE_ORIGIN_FRONT_ELEMENT = 1 } lf_flare_origin;" in header
    assert (pkg.FLARE_ORIGIN_CAMERA, pkg.FLARE_ORIGIN_FRONT_ELEMENT) == (CAMERA, FRONT)
    for name in ("set_flare_occlusion", "get_flare_occlusion", "flare_visibility"):
        assert callable(getattr(pkg.LensFlare, name)), name
    assert callable(pkg.flare_shadow_samples) and callable(pkg.flare_shadow_rays)
    # the ghost occlusion contract points here instead of listing the flare layer as missing
    assert "Not covered" not in header and "lf_set_flare_occlusion (below) hides them" in header


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper reached the library ({name}) with arguments it should have refused")


def _bare(pkg):
    lf = pkg.LensFlare.__new__(pkg.LensFlare)
    lf.lib, lf.ctx, lf._owned = _NoLibrary(), C.c_void_p(), False
    return lf


REFUSED = [dict(rays_per_light=63), dict(rays_per_light=65), dict(rays_per_light=4160), dict(rays_per_light=0),
           dict(angular_radius=-1e-6), dict(angular_radius=0.5001), dict(angular_radius=float("nan")),
           dict(origin=2), dict(origin=-1),
           dict(origin=FRONT, world_per_mm=0.0), dict(origin=FRONT, world_per_mm=-0.001), dict(origin=FRONT, world_per_mm=float("inf")),
           dict(origin=FRONT, world_per_mm=float("nan"))]


def test_the_wrapper_refuses_what_the_contract_refuses_without_a_device():
    pkg = _pkg()
    lf = _bare(pkg)
    good = dict(rays_per_light=256, angular_radius=ALPHA, origin=CAMERA, world_per_mm=WPM)
    for bad in REFUSED:
        with pytest.raises(ValueError):
            lf.set_flare_occlusion(True, **{**good, **bad})
    # ... and what is fine does reach it: the limits themselves, a scale that CAMERA ignores, switching off
    for ok in (dict(rays_per_light=64), dict(rays_per_light=4096), dict(angular_radius=0.0), dict(angular_radius=0.5),
               dict(origin=CAMERA, world_per_mm=-1.0), dict(origin=FRONT)):
        with pytest.raises(AssertionError):
            lf.set_flare_occlusion(True, **{**good, **ok})
    with pytest.raises(AssertionError):
        lf.set_flare_occlusion(False, rays_per_light=63)
    # the host functions refuse the same in the library itself (no context: no device needed)
    lib = pkg.load_library()
    out = np.zeros(4 * 4160, np.float32)
    fo = np.array([0.5, 0.5], np.float64)
    rays = np.zeros(6 * 4160, np.float32)
    fp, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    for R in (63, 65, 4160, 0, -64):
        assert lib.lf_flare_shadow_samples(C.c_int(R), fp(out)) == 1, R
        assert lib.lf_flare_shadow_rays(C.c_int(R), dp(fo), C.c_double(HFOV), C.c_double(VFOV), C.c_float(ALPHA), CAMERA, C.c_float(0), fp(rays)) == 1
    call = lambda a, o, h: lib.lf_flare_shadow_rays(C.c_int(64), dp(fo), C.c_double(HFOV), C.c_double(VFOV), C.c_float(a), C.c_int(o), C.c_float(h), fp(rays))
    assert call(ALPHA, CAMERA, 0.0) == 0 and call(ALPHA, FRONT, 17.0) == 0
    for a, o, h in ((-1e-6, CAMERA, 0.0), (0.5001, CAMERA, 0.0), (float("nan"), CAMERA, 0.0), (ALPHA, 2, 0.0), (ALPHA, -1, 0.0), (ALPHA, FRONT, 0.0)):
        assert call(a, o, h) == 1, (a, o, h)


def test_the_samples_are_the_stated_set():
    pkg = _pkg()
    for R in (64, 256, 1024, 4096):
        t = pkg.flare_shadow_samples(R).astype(np.float64)
        assert t.shape == (R, 4)
        ra2, rl2 = t[:, 0] ** 2 + t[:, 1] ** 2, t[:, 2] ** 2 + t[:, 3] ** 2
        assert (ra2 <= 1.0).all() and (rl2 <= 1.0).all()        # inside the unit discs
        # u0 = (r + 0.5) / R: exactly one aperture sample per ring of equal area, in order
        assert np.array_equal(np.floor(ra2 * R).astype(int), np.arange(R))
        # ... and the float64 restatement to 1 float ulp (sin and cos are libm's)
        ref = samples64(R)
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        assert (np.abs(t - ref) <= ulp).all(), float((np.abs(t - ref) / ulp).max())
        # the light's disc is covered, not clustered: every quadrant holds its share within a quarter of it
        quad = (t[:, 2] > 0).astype(int) * 2 + (t[:, 3] > 0).astype(int)
        assert (np.abs(np.bincount(quad, minlength=4) - R / 4) <= R / 16).all()


def test_the_rays_are_the_float64_restatement_bit_for_bit():
    pkg = _pkg()
    h0 = float(pkg.load_lens_file("dgauss11.lens")["semi_aperture"][0])
    for R in (64, 1024):
        table = pkg.flare_shadow_samples(R)
        for flare in FLARES:
            for origin in (CAMERA, FRONT):
                got = pkg.flare_shadow_rays(R, flare, HFOV, VFOV, ALPHA, origin, h0)
                want = rays64(table, flare, ALPHA, origin, h0)
                assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (R, flare, origin)
                assert np.array_equal(got[:, 2], np.zeros(R, np.float32))
                if origin == CAMERA:
                    assert not got[:, :3].any()
                else:
                    assert (np.hypot(got[:, 0], got[:, 1]) <= h0 * (1 + 1e-6)).all() and np.abs(got[:, :2]).max() > 0.9 * h0
                # the directions lie within alpha of s (unnormalised: s + tan(alpha) times a point of the unit disc)
                s, _, _ = flare_dir64(flare)
                off = np.linalg.norm(got[:, 3:].astype(np.float64) - s[None, :], axis=1)
                assert (off <= np.tan(ALPHA) * (1 + 1e-5) + 1e-7).all() and off.max() > 0.9 * np.tan(ALPHA)
            # alpha = 0: every direction is s itself
            flat = pkg.flare_shadow_rays(R, flare, HFOV, VFOV, 0.0, CAMERA)
            assert (flat[:, 3:] == flat[0, 3:]).all()
            assert np.array_equal(flat[0, 3:], flare_dir64(flare)[0].astype(np.float32))
    # the flare at the centre of the frame looks straight down -z
    assert np.array_equal(pkg.flare_shadow_rays(64, (0.5, 0.5), HFOV, VFOV, 0.0, CAMERA)[0, 3:], np.array([0, 0, -1], np.float32))


def test_the_wall_of_the_device_test_has_no_fragile_ray():
    """The device test counts rays against a wall whose edge crosses each beam (tests/test_gpu_flare_occlusion.py).  On the
    CPU, with the double-Gauss lens' entrance pupil: every ray's margin to an edge is >= 1e-9 up to R = 4096, the wall
    blocks a fraction well inside (0, 1), and a wrong mapping counts differently."""
    pkg = _pkg()
    lens = pkg.load_lens_file("dgauss11.lens")
    h0 = float(lens["semi_aperture"][0])
    z_ref, _ = pkg.paraxial_entrance_pupil(lens)
    smallest = np.inf
    mutants = dict(x_flipped=dict(x_flip=-1.0), z_ref_dropped=dict(use_z_ref=False), wpm_squared=dict(wpm_power=2))
    for R in (64, 256, 1024, 4096):
        right, wrong = [], {name: [] for name in mutants}
        for flare in FLARES:
            for origin in (CAMERA, FRONT):
                rays = pkg.flare_shadow_rays(R, flare, HFOV, VFOV, ALPHA, origin, h0)
                cx = beam_centre_x(flare, -0.8, origin, WPM, z_ref)
                wall = (-0.8, cx - 0.5, cx + 0.0013, -0.6, 0.7)
                hit, margin = quad_margin(*shadow_ray64(rays, WPM if origin == FRONT else 1.0, z_ref if origin == FRONT else 0.0), *wall)
                smallest = min(smallest, float(margin.min()))
                assert margin.min() >= 1e-9, (R, flare, origin, float(margin.min()))
                # the wall covers everything left of the beam's centre and 1.3 mm beyond it, the beam is at least
                # 0.8 tan(alpha) = 3.7 mm wide: more than half of the rays are blocked, not all of them
                assert 0.5 < hit.mean() < 1.0, (R, flare, origin, float(hit.mean()))
                if origin == FRONT:
                    right.append(int(hit.sum()))
                    for name, kw in mutants.items():
                        wrong[name].append(int(quad_margin(*shadow_ray64(rays, WPM, z_ref, **kw), *wall)[0].sum()))
        # a wrong mapping counts differently (over the three flares: on the axis z_ref only moves the origin along the beam)
        for name in mutants:
            assert wrong[name] != right, (R, name, right)
            assert sum(a != b for a, b in zip(wrong[name], right)) >= 2, (R, name, wrong[name], right)
    assert smallest >= 1e-9


def test_the_frame_plan_carries_the_setting_and_the_mirrors_install_it():
    seq = open(os.path.join(HOST, "lf_frame_sequence.h")).read()
    for field in ("int flare_occlusion;", "int flare_occlusion_rays;", "int flare_occlusion_origin;"):
        assert re.search(re.escape(field) + r"[^}]*\}\s*lf_frame_plan;", seq, re.S), field
    assert re.search(r"lf_set_flare_occlusion\(ctx, p->flare_occlusion \? 1 : 0, p->flare_occlusion_rays, p->sun_angular_radius,\s*"
                     r"p->flare_occlusion_origin, p->world_per_mm\)", seq)
    assert seq.index("lf_set_flare_occlusion(ctx") < seq.index("lf_trace_ghosts(ctx") < seq.index("lf_render_flare_layer(ctx")
    dropin = open(os.path.join(HOST, "pathtracer_amd.cpp")).read()
    assert re.findall(r"plan\.flare_occlusion\s*=\s*([^;]+);", dropin) == ["0"]
    mirror = open(os.path.join(HOST, "lf_pathtracer.cpp")).read()
    assert re.findall(r"plan\.flare_occlusion\s*=\s*([^;]+);", mirror) == ["flare_occlusion_ ? 1 : 0"]
    assert re.search(r"void use_flare_occlusion\(bool on, int rays = 1024\);", open(os.path.join(HOST, "lf_pathtracer.h")).read())
    assert "flarewall" in open(os.path.join(HOST, "shim_demo.cpp")).read()
