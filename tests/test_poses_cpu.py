"""Posed interfaces (decentred, tilted, rotated: lf_set_lens_poses), host side (no device): the float32 event the kernels run
(lf_pose_event, lf_pose.h) against the float64 tracer of tests/pose_ref.py -- closed forms, the identities of the event, its
accuracy on the posed interfaces of data/dgauss11_decentred.lens and on one general case (a tilted, decentred, rotated
biconic), pose_group against the rigid body, the shipped lens and the Python parser.

THE YARDSTICK is tests/test_biconics_cpu.py's: D is the deviation of the float32 spherical event that exists (the oracle's
geo_glass_event) from float64 on the same rays through the sphere of the stronger meridian's curvature; the bar is 4 D.  The
acceptance rule and its bands (the rim, the critical angle) are that file's; a posed event has one band more, the rays whose
local K'_z is within the bar of zero (their side of the surface is not float32's to decide).  D and the worst deviation per
case, in multiples of D, go to profiles/pose_accuracy.json.

The setter, the getter, the refusals and the C parser need a context, which needs a device: tests/test_gpu_poses.py covers them."""
import importlib.util
import json
import os

import numpy as np
import pytest

import asphere_ref as ar
import biconic_ref as br
import pose_ref as pr
import test_biconics_cpu as tb
from test_aspheres_cpu import _pkg, COS_MIN, N_RAYS, ROOT

DATA = os.path.join(ROOT, "lens-flare_amd", "data")
_cache = {}


def _f32(v):
    return float(np.float32(v))


def _lens():
    if "lens" not in _cache:
        _cache["lens"] = _pkg().load_lens_file("dgauss11_decentred.lens")
    return _cache["lens"]


def _cases():
    """the posed interfaces of the shipped lens (a rotated toroid, the three faces of the decentred, tilted doublet) and a
    general case: test_biconics_cpu's general biconic, decentred in x, y and z and turned about all three axes.  (The names
    are this file's own: test_biconics_cpu caches D by name, and its cases are called interface_1, interface_2 and general.)"""
    if "cases" in _cache:
        return _cache["cases"]
    lens = _lens()
    G = pr.lens_geometry(lens)
    out = []
    for k in range(G["n"]):
        if not G["pose_on"][k]:
            continue
        cy = _f32(np.float32(1.0) / np.float32(lens["radius"][k]))
        cx = _f32(np.float32(1.0) / np.float32(lens["biconics"]["radius_x"][k])) if G["bic_on"][k] else cy
        before = k - 1 if k - 1 != G["stop"] else k - 2
        out.append(dict(name=f"posed_interface_{k}", cx=cx, cy=cy, kx=0.0, ky=0.0, h=float(G["h"][k]),
                        n_before=1.0 if before < 0 else float(G["ior"][1][before]), n_after=float(G["ior"][1][k]),
                        t=[_f32(v) for v in G["pose_t"][k]], a=[_f32(v) for v in G["pose_a"][k]]))
    g = tb._cases()[-1]
    out.append(dict(g, name="posed_general", t=[_f32(0.8), _f32(-0.5), _f32(0.3)], a=[6.0, -4.0, 35.0]))
    _cache["cases"] = out
    return out


def _surface(s):
    return pr.surface("bic", cx=s["cx"], cy=s["cy"], kx=s["kx"], ky=s["ky"])


def _host(s, t, a, reflect, forward, z0, p, d, n_in, n_out, asphere=None):
    """lf_pose_event on rays (p, unit d) that start in the plane z0 from the nominal vertex, in the medium n_in"""
    rays = np.concatenate([p[:, :2], np.zeros((len(p), 1), np.float32), d * np.float32(n_in)], axis=1).astype(np.float32)
    return _pkg().pose_event(s["cx"], s["cy"], s["kx"], s["ky"], asphere, t, a, s["h"], np.float32(n_in), np.float32(n_out),
                             reflect, forward, z0, rays)


def _run(s, forward, reflect, seed, t=None, a=None):
    """the float32 posed event and the float64 one on test_biconics_cpu's rays (lens coordinates: the same rays D is measured on)"""
    t = s["t"] if t is None else t
    a = s["a"] if a is None else a
    p, d, z0 = tb._rays(s, forward, seed)
    n_in, n_out = (s["n_before"], s["n_after"]) if forward else (s["n_after"], s["n_before"])
    n_in32, n_out32 = np.float32(n_in), np.float32(n_out)
    out, fates = _host(s, t, a, reflect, forward, z0, p, d, n_in32, n_out32)
    ref = pr.event(p, d, (0.0, 0.0, 0.0), _surface(s), s["h"], t, a, float(n_in32), float(n_out32), bool(reflect), bool(forward))
    n_leave = n_in32 if reflect else n_out32
    return dict(out=out, fates=fates, ref=ref, d32=out[:, 3:6].astype(np.float64) / float(n_leave), n_in=float(n_in32),
                n_out=float(n_out32), p=p, d=d, z0=z0)


def _bands(s, r, bar, reflect):
    clear, k, k_band = tb._bands(s, r, bar, reflect)
    return clear & (r["ref"]["towards_margin"] > bar), k, k_band


def dump_rays(path):
    """the rays of the accuracy test -- every case, direction and event, and the general case once more as a sphere with an
    aspheric record -- as the binary file profiles/pose_sanitizer.hip reads (the host event under the sanitizers)"""
    import struct
    c = _f32(np.float32(1.0) / np.float32(30.0))
    recs = []
    for s, asph in [(s, 0) for s in _cases()] + [(dict(_cases()[-1], cx=c, cy=c, kx=0.0, ky=0.0), 1)]:
        for forward in (0, 1):
            for reflect in (0, 1):
                p, d, z0 = tb._rays(s, forward, 10 + 2 * forward + reflect)
                n_in, n_out = (s["n_before"], s["n_after"]) if forward else (s["n_after"], s["n_before"])
                for i in range(len(p)):
                    ray = [p[i, 0], p[i, 1], 0.0] + [float(np.float32(v) * np.float32(n_in)) for v in d[i]]
                    recs.append(struct.pack("<8f3i12f", s["cx"], s["cy"], s["kx"], s["ky"], s["h"], n_in, n_out, float(z0), reflect,
                                            forward, asph, *s["t"], *s["a"], *ray))
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(recs)))
        f.write(b"".join(recs))
    return len(recs)


# ---------------------------------------------------------------- closed forms --------------------------------------------------
PLANE = dict(name="plane", cx=0.0, cy=0.0, kx=0.0, ky=0.0, h=20.0)


def _bar():
    """the bar of the closed forms and the identities: 4 D of the general case's biconic (test_biconics_cpu's)"""
    return 4 * tb._D(tb._cases()[-1])


def _axial(z0=-5.0):
    return np.array([[0.0, 0.0, z0]], np.float32), np.array([[0.0, 0.0, 1.0]], np.float32)


@pytest.mark.parametrize("theta", [3.0, 12.5, 25.0])
def test_a_tilted_plate_displaces_a_ray_and_leaves_its_direction(theta):
    """d sin(theta) (1 - cos(theta) / sqrt(n^2 - sin^2(theta))), towards the side the plate's normal leans to: the plate is
    tilted by ax = theta about its first vertex, its normal (0, -sin, cos) -- the ray bends towards it inside: -y"""
    n, thick = _f32(1.6), 4.0
    th = np.deg2rad(theta)
    want = thick * np.sin(th) * (1.0 - np.cos(th) / np.sqrt(n * n - np.sin(th) ** 2))
    R = pr.rotation([theta, 0, 0])
    t2 = (R - np.eye(3)) @ np.array([0.0, 0.0, thick])          # the second face of the rigid plate
    p, d = _axial()
    # float64
    e1 = pr.event(p, d, (0, 0, 0), _surface(PLANE), PLANE["h"], (0, 0, 0), (theta, 0, 0), 1.0, n, False, True)
    e2 = pr.event(e1["p"], e1["d"], (0, 0, thick), _surface(PLANE), PLANE["h"], t2, (theta, 0, 0), n, 1.0, False, True)
    assert e2["fate"][0] == pr.ALIVE
    assert abs(e2["p"][0, 1] + want) < 1e-12 and abs(e2["p"][0, 0]) < 1e-12
    assert np.max(np.abs(e2["d"][0] - [0, 0, 1])) < 1e-12
    # float32: the two events chained as the march chains them (z from each interface's nominal vertex)
    o1, f1 = _host(PLANE, (0, 0, 0), (theta, 0, 0), 0, 1, np.float32(-5.0), p, d, 1.0, n)
    rays2 = o1[:, :6].copy()
    o2, f2 = _pkg().pose_event(0, 0, 0, 0, None, t2, (theta, 0, 0), PLANE["h"], np.float32(n), np.float32(1.0), 0, 1, np.float32(-thick), rays2)
    assert f1[0] == 0 and f2[0] == 0
    bar = _bar()
    assert abs(o2[0, 1] + want) <= bar and abs(o2[0, 0]) <= bar
    assert np.max(np.abs(o2[0, 3:6] - [0, 0, 1])) <= bar
    assert abs(o2[0, 1]) > 100 * bar                             # (the displacement is no rounding)


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("beta", [-7.0, 2.0, 11.0])
def test_a_tilted_mirror_turns_the_ray_by_twice_its_tilt(axis, beta):
    """the axial ray (0, 0, 1) comes back as Rx(2 beta) (0, 0, -1) = (0, sin 2b, -cos 2b) for ax = beta and as
    Ry(2 beta) (0, 0, -1) = (-sin 2b, 0, -cos 2b) for ay = beta"""
    b2 = np.deg2rad(2 * beta)
    want = np.array([0.0, np.sin(b2), -np.cos(b2)]) if axis == 0 else np.array([-np.sin(b2), 0.0, -np.cos(b2)])
    tilt = [beta, 0, 0] if axis == 0 else [0, beta, 0]
    p, d = _axial()
    e = pr.event(p, d, (0, 0, 0), _surface(PLANE), PLANE["h"], (0, 0, 0), tilt, 1.0, 1.5, True, True)
    assert e["fate"][0] == pr.ALIVE and np.max(np.abs(e["d"][0] - want)) < 1e-12
    o, f = _host(PLANE, (0, 0, 0), tilt, 1, 1, np.float32(-5.0), p, d, 1.0, 1.5)
    assert f[0] == 0 and np.max(np.abs(o[0, 3:6] - want)) <= _bar()
    # the same on a curved mirror's vertex: the tilt turns the normal there
    sph = dict(PLANE, cx=_f32(1 / 40.0), cy=_f32(1 / 40.0))
    o, f = _host(sph, (0, 0, 0), tilt, 1, 1, np.float32(-5.0), p, d, 1.0, 1.5)
    assert f[0] == 0 and np.max(np.abs(o[0, 3:6] - want)) <= _bar()


@pytest.mark.parametrize("alpha", [-9.0, 4.0, 15.0])
def test_a_wedge_deviates_the_ray_by_snells_law(alpha):
    """normal incidence on the first face, incidence alpha on the second (ax = alpha: its normal (0, -sin a, cos a)):
    the exit ray leaves at asin(n sin a) from that normal, on the incident ray's side -- (0, sin d, cos d), d = asin(n sin a) - a"""
    n = _f32(1.5)
    al = np.deg2rad(alpha)
    dev = np.arcsin(n * np.sin(al)) - al
    want = np.array([0.0, np.sin(dev), np.cos(dev)])
    p, d = _axial()
    e1 = pr.event(p, d, (0, 0, 0), _surface(PLANE), PLANE["h"], (0, 0, 0), (0, 0, 0), 1.0, n, False, True)
    e2 = pr.event(e1["p"], e1["d"], (0, 0, 3.0), _surface(PLANE), PLANE["h"], (0, 0, 0), (alpha, 0, 0), n, 1.0, False, True)
    assert e2["fate"][0] == pr.ALIVE and np.max(np.abs(e2["d"][0] - want)) < 1e-12
    o1, f1 = _host(PLANE, (0, 0, 0), (0, 0, 0), 0, 1, np.float32(-5.0), p, d, 1.0, n)
    o2, f2 = _pkg().pose_event(0, 0, 0, 0, None, (0, 0, 0), (alpha, 0, 0), PLANE["h"], np.float32(n), np.float32(1.0), 0, 1,
                               np.float32(-3.0), o1[:, :6].copy())
    assert f1[0] == 0 and f2[0] == 0 and np.max(np.abs(o2[0, 3:6] - want)) <= _bar()


# ---------------------------------------------------------------- identities of the host event ----------------------------------
def test_a_record_of_zeros_is_the_biconic_route_bit_for_bit():
    pkg = _pkg()
    c = _f32(np.float32(1.0) / np.float32(30.0))
    for s in (dict(tb._cases()[-1]), dict(PLANE, n_before=1.0, n_after=_f32(1.6)),
              dict(name="sphere", cx=c, cy=c, kx=0.0, ky=0.0, h=12.0, n_before=1.0, n_after=_f32(1.6)),
              dict(name="cylinder", cx=c, cy=0.0, kx=0.0, ky=0.0, h=12.0, n_before=1.0, n_after=_f32(1.6))):
        for forward in (0, 1):
            for reflect in (0, 1):
                p, d, z0 = tb._rays(s, forward, 50 + 2 * forward + reflect)
                n_in, n_out = (s["n_before"], s["n_after"]) if forward else (s["n_after"], s["n_before"])
                rays = np.concatenate([p[:, :2], np.zeros((len(p), 1), np.float32), d * np.float32(n_in)], axis=1).astype(np.float32)
                o1, f1 = pkg.pose_event(s["cx"], s["cy"], s["kx"], s["ky"], None, (0, 0, 0), (0, 0, 0), s["h"], np.float32(n_in),
                                        np.float32(n_out), reflect, forward, z0, rays)
                o2, f2 = pkg.biconic_event(s["cx"], s["cy"], s["kx"], s["ky"], s["h"], np.float32(n_in), np.float32(n_out), reflect,
                                           forward, z0, rays)
                assert np.array_equal(f1, f2), s["name"]
                live = f1 == 0
                assert live.sum() > 100 and np.array_equal(o1[live], o2[live]), s["name"]


def _compare(name, s, r, out2, fates2, bar, reflect):
    """two float32 events on the same rays: within the bar of each other where float64 is clear of every band"""
    clear, k, k_band = _bands(s, r, bar, reflect)
    assert clear.sum() > 300, name
    assert np.all(r["fates"][clear] == 0) and np.all(fates2[clear] == 0), name
    dev = np.abs(r["out"][clear, :6].astype(np.float64) - out2[clear, :6].astype(np.float64))
    assert dev.max() <= bar, (name, float(dev.max()), bar)
    return float(dev.max())


def test_a_turn_about_z_leaves_a_surface_of_revolution_alone():
    c = _f32(np.float32(1.0) / np.float32(30.0))
    s = dict(name="sphere", cx=c, cy=c, kx=0.0, ky=0.0, h=12.0, n_before=1.0, n_after=_f32(1.6), t=[0, 0, 0], a=[0, 0, 0])
    bar = 4 * tb._D(s)
    for forward in (0, 1):
        for reflect in (0, 1):
            r = _run(s, forward, reflect, 60 + 2 * forward + reflect)
            for az in (37.0, -120.0):
                o2, f2 = _host(s, (0, 0, 0), (0, 0, az), reflect, forward, r["z0"], r["p"], r["d"], r["n_in"], r["n_out"])
                _compare("sphere az", s, r, o2, f2, bar, reflect)
                # ... and an aspheric record (the conicoid of the same vertex curvature)
                asph = (-0.6, [1e-6])
                o3, f3 = _host(s, (0, 0, 0), (0, 0, 0), reflect, forward, r["z0"], r["p"], r["d"], r["n_in"], r["n_out"], asph)
                o4, f4 = _host(s, (0, 0, 0), (0, 0, az), reflect, forward, r["z0"], r["p"], r["d"], r["n_in"], r["n_out"], asph)
                both = (f3 == 0) & (f4 == 0) & _bands(s, r, bar, reflect)[0]
                assert both.sum() > 300 and np.max(np.abs(o3[both, :6].astype(np.float64) - o4[both, :6])) <= bar


def test_a_quarter_turn_swaps_a_cylinders_meridians():
    """az = 90 on a cylinder with power in x is the cylinder with power in y"""
    c = _f32(np.float32(1.0) / np.float32(30.0))
    sx = dict(name="cyl_x", cx=c, cy=0.0, kx=0.0, ky=0.0, h=12.0, n_before=1.0, n_after=_f32(1.6), t=[0, 0, 0], a=[0, 0, 90.0])
    sy = dict(sx, name="cyl_y", cx=0.0, cy=c, a=[0, 0, 0])
    bar = 4 * tb._D(sx)
    for forward in (0, 1):
        for reflect in (0, 1):
            r = _run(sx, forward, reflect, 70 + 2 * forward + reflect)          # (float64 follows the TURNED x cylinder)
            o2, f2 = _host(sy, (0, 0, 0), (0, 0, 0), reflect, forward, r["z0"], r["p"], r["d"], r["n_in"], r["n_out"])
            _compare("quarter turn", sx, r, o2, f2, bar, reflect)
            # (the power IS in y now: the un-turned x cylinder is far away)
            o3, f3 = _host(sx, (0, 0, 0), (0, 0, 0), reflect, forward, r["z0"], r["p"], r["d"], r["n_in"], r["n_out"])
            both = (f3 == 0) & (r["fates"] == 0)
            assert np.max(np.abs(o3[both, :6].astype(np.float64) - r["out"][both, :6])) > 1000 * bar


def test_a_decentre_is_the_centred_event_on_the_shifted_ray():
    """(dx, dy): the ray shifted by (-dx, -dy), the centred event, the result shifted back -- in float32, bit for bit"""
    s = dict(tb._cases()[-1])
    t = np.array([_f32(0.7), _f32(-1.3), 0.0], np.float32)
    for forward in (0, 1):
        for reflect in (0, 1):
            p, d, z0 = tb._rays(s, forward, 80 + 2 * forward + reflect)
            n_in, n_out = (s["n_before"], s["n_after"]) if forward else (s["n_after"], s["n_before"])
            o1, f1 = _host(s, t, (0, 0, 0), reflect, forward, z0, p, d, n_in, n_out)
            ps = p.copy()
            ps[:, 0] = p[:, 0] - t[0]; ps[:, 1] = p[:, 1] - t[1]
            o2, f2 = _host(s, (0, 0, 0), (0, 0, 0), reflect, forward, z0, ps, d, n_in, n_out)
            assert np.array_equal(f1, f2)
            live = f1 == 0
            back = o2.copy()
            back[:, 0] = o2[:, 0] + t[0]; back[:, 1] = o2[:, 1] + t[1]
            assert live.sum() > 300 and np.array_equal(o1[live], back[live])
            assert np.max(np.abs(o1[live, :2] - o2[live, :2])) > 0.5          # (the shift is there)


# ---------------------------------------------------------------- accuracy ------------------------------------------------------
def test_the_posed_event_against_float64_and_the_acceptance_rule():
    record = {}
    for s in _cases():
        D = tb._D(s)
        bar = 4 * D
        worst = 0.0
        counts = dict(rays=0, compared=0)
        for forward in (0, 1):
            for reflect in (0, 1):
                r = _run(s, forward, reflect, 10 + 2 * forward + reflect)
                ref, fates = r["ref"], r["fates"]
                clear, k, k_band = _bands(s, r, bar, reflect)
                counts["rays"] += len(fates); counts["compared"] += int(clear.sum())
                assert clear.sum() > 300
                # every ray float64 accepts clear of the bands is accepted ...
                assert np.all(fates[clear] == 0), (s["name"], forward, reflect, np.unique(fates[clear], return_counts=True))
                # ... no accepted ray is farther than the bar from the float64 hit (position and direction) ...
                both = (fates == 0) & (ref["fate"] == ar.ALIVE) & (ref["cos_i"] > COS_MIN)
                dev = np.maximum(np.max(np.abs(r["out"][both, 0:3] - ref["p"][both]), axis=1),
                                 np.max(np.abs(r["d32"][both] - ref["d"][both]), axis=1))
                worst = max(worst, float(dev.max()))
                # ... an accepted ray float64 rejects lies within the bar of the rim or of the critical angle ...
                odd = (fates == 0) & (ref["fate"] != ar.ALIVE) & (r["out"][:, 6] > COS_MIN * r["n_in"])
                assert np.all(ref["fate"][odd] != ar.MISSED), "float32 accepts a ray that misses the surface in float64"
                assert np.all((ref["rim"][odd] <= bar) | (np.abs(k[odd]) <= k_band))
                # ... and what misses in float64 is dead in float32
                assert np.all(fates[ref["fate"] == ar.MISSED] != 0)
        print(f"{s['name']}: D = {D:.3e}, posed event's worst deviation = {worst:.3e} ({worst / D:.2f} D)")
        record[s["name"]] = dict(cx=s["cx"], cy=s["cy"], kx=s["kx"], ky=s["ky"], decentre=s["t"], tilt_deg=s["a"], D=D, bar=bar,
                                 pose_worst=worst, pose_worst_in_D=worst / D, **counts)
        assert worst <= bar, (s["name"], worst, bar)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pose_accuracy.json"), "w") as f:
        json.dump(dict(what="float32 posed event (lf_pose_event) vs the float64 tracer of tests/pose_ref.py on the posed interfaces "
                            "of data/dgauss11_decentred.lens and a general case (a tilted, decentred, rotated biconic); D: the "
                            "oracle's spherical event on the sphere of the stronger meridian's curvature (existing code) on the "
                            "same rays, pose_worst: lf_pose_event; mm and unit-direction components, the larger of the two; the "
                            "bar is 4 D",
                       rays_per_case=N_RAYS, cos_min=COS_MIN, **record), f, indent=1)
        f.write("\n")


def test_the_general_case_moves_the_hit_by_1000_bars():
    s = _cases()[-1]
    r = _run(s, 1, 0, 10 + 2)
    c = _run(s, 1, 0, 10 + 2, t=[0, 0, 0], a=[0, 0, 0])
    both = (r["fates"] == 0) & (c["fates"] == 0)
    assert np.median(np.max(np.abs(r["out"][both, :3] - c["out"][both, :3]), axis=1)) > 1000 * 4 * tb._D(s)


# ---------------------------------------------------------------- pose_group ----------------------------------------------------
def test_pose_group_is_the_rigid_body():
    """a two-face element (a biconvex singlet) tilted about a pivot on the axis and decentred: the records of pose_group, fed
    to the host event face by face, against pose_ref tracing the BODY -- each face's vertex carried to
    pivot + d + R (V_k - pivot) here, with no decentre of its own"""
    pkg = _pkg()
    glass = _f32(1.6)
    c1, c2 = _f32(np.float32(1.0) / np.float32(40.0)), _f32(np.float32(1.0) / np.float32(-55.0))
    thick, h = 5.0, 10.0
    lens = dict(n=2, stop=-1, radius=np.array([40.0, -55.0], np.float32), thickness=np.array([thick, 30.0], np.float32),
                ior=np.array([[glass, 1.0]], np.float32), semi_aperture=np.array([h, h], np.float32), sensor_width_mm=36.0)
    pivot, dec, tilt = 2.0, np.array([0.4, -0.25, 0.1]), [3.0, -2.0, 0.0]
    rec = pkg.pose_group(lens, 0, 1, pivot, dec, tilt)
    assert rec["on"].tolist() == [1, 1] and np.array_equal(rec["tilt_deg"], np.array([tilt, tilt], np.float32))
    assert not np.array_equal(rec["decentre"][0], rec["decentre"][1])          # (the faces need different records)
    R = pr.rotation(tilt)
    V = [np.array([0.0, 0.0, pivot]) + dec + R @ (np.array([0.0, 0.0, z]) - np.array([0.0, 0.0, pivot])) for z in (0.0, thick)]
    s1 = dict(name="face0", cx=c1, cy=c1, kx=0.0, ky=0.0, h=h, n_before=1.0, n_after=glass)
    s2 = dict(name="face1", cx=c2, cy=c2, kx=0.0, ky=0.0, h=h, n_before=glass, n_after=1.0)
    bar = 4 * tb._D(s1)
    p, d, z0 = tb._rays(s1, 1, 90)
    # float64: the body
    e1 = pr.event(p, d, V[0], _surface(s1), h, (0, 0, 0), tilt, 1.0, glass, False, True)
    e2 = pr.event(e1["p"], e1["d"], V[1], _surface(s2), h, (0, 0, 0), tilt, glass, 1.0, False, True)
    # float32: pose_group's records
    o1, f1 = _host(s1, rec["decentre"][0], rec["tilt_deg"][0], 0, 1, z0, p, d, 1.0, glass)
    o2, f2 = pkg.pose_event(c2, c2, 0, 0, None, rec["decentre"][1], rec["tilt_deg"][1], h, np.float32(glass), np.float32(1.0), 0, 1,
                            np.float32(-thick), o1[:, :6].copy())
    ok = (e1["fate"] == pr.ALIVE) & (e2["fate"] == pr.ALIVE) & (np.minimum(e1["rim"], e2["rim"]) > 2 * bar) & \
         (np.minimum(e1["cos_i"], e2["cos_i"]) > COS_MIN)
    k2 = 1.0 - glass ** 2 * (1.0 - e2["cos_i"] ** 2)
    ok &= k2 > 0.05
    assert ok.sum() > 300 and np.all(f1[ok] == 0) and np.all(f2[ok] == 0)
    got_p = o2[ok, :3].astype(np.float64) + [0.0, 0.0, thick]                  # (z from face 1's nominal vertex)
    assert np.max(np.abs(got_p - e2["p"][ok])) <= 2 * bar                       # (two events)
    assert np.max(np.abs(o2[ok, 3:6] - e2["d"][ok])) <= 2 * bar
    # ... and pose_group's rule, by hand
    for k, z in enumerate((0.0, thick)):
        assert np.allclose(rec["decentre"][k], dec + (R - np.eye(3)) @ np.array([0.0, 0.0, z - pivot]), atol=1e-6)


# ---------------------------------------------------------------- the shipped lens and the Python parser ------------------------
def test_the_shipped_lens_is_what_its_script_writes():
    spec = importlib.util.spec_from_file_location("make_decentred_lens", os.path.join(DATA, "make_decentred_lens.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.generate(open(os.path.join(DATA, "dgauss11.lens")).read()) == open(os.path.join(DATA, "dgauss11_decentred.lens")).read()
    pkg = _pkg()
    lens, base = _lens(), pkg.load_lens_file("dgauss11.lens")
    for key in ("radius", "thickness", "ior", "semi_aperture"):
        assert np.array_equal(lens[key], base[key])
    po = lens["poses"]
    assert po["on"].tolist() == [0, 1, 1, 1, 1] + [0] * 6 and lens["biconics"]["on"].tolist() == [0, 1] + [0] * 9
    assert np.array_equal(po["tilt_deg"][1], np.array([0, 0, 30], np.float32))          # the rotated cylinder
    # the doublet: pose_group's records about its front vertex, a fraction of a millimetre and of a degree
    z2 = float(np.sum(base["thickness"][:2].astype(np.float64)))
    rec = pkg.pose_group(base, 2, 4, z2, m.GROUP_DECENTRE, m.GROUP_TILT)
    assert np.allclose(po["decentre"][2:5], rec["decentre"][2:5], atol=1e-6) and np.array_equal(po["tilt_deg"][2:5], rec["tilt_deg"][2:5])
    assert 0 < np.max(np.abs(po["decentre"][2:5])) < 1.0 and 0 < np.max(np.abs(po["tilt_deg"][2:5])) < 1.0


def test_the_python_parser_refuses_what_the_setter_refuses(tmp_path):
    pkg = _pkg()
    base = open(os.path.join(DATA, "dgauss11.lens")).read()
    def load(extra):
        f = tmp_path / "x.lens"
        f.write_text(base + extra)
        return pkg.load_lens_file(str(f))
    ok = load("pose 3 0.1 0 0 1 2 3\n")
    assert ok["poses"]["on"][3] == 1 and np.array_equal(ok["poses"]["tilt_deg"][3], np.array([1, 2, 3], np.float32))
    assert "poses" not in load("")
    for bad in ("pose 3 0.1 0 0 1 2\n", "pose 3 0.1 0 0 1 2 3 4\n", "pose 11 0 0 0 0 0 0\n", "pose -1 0 0 0 0 0 0\n",
                "pose 3 0 0 0 0 0 0\npose 3 0 0 0 0 0 0\n", "pose 5 0 0 0 0 0 0\n", "pose 3 0 0 0 31 0 0\n", "pose 3 0 0 0 0 -30.5 0\n",
                "pose 3 0 0 0 0 0 181\n", "pose 3 nan 0 0 0 0 0\n"):
        with pytest.raises(ValueError):
            load(bad)
