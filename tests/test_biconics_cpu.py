"""Biconic interfaces, host side (no device): the float32 event the kernels run (lf_biconic_event, lf_biconic.h) against the
float64 tracer of tests/biconic_ref.py -- on the two cylinder faces of data/dgauss11_anamorphic.lens and on one synthetic
general biconic -- its degenerate identities, the shipped lens and the Python parser.

THE YARDSTICK is tests/test_aspheres_cpu.py's: D is the deviation of the float32 spherical event that exists (the oracle's
geo_glass_event) from float64 on the same rays through the SPHERE OF THE STRONGER MERIDIAN'S CURVATURE; the bar is 4 D.  The
acceptance rule and its two bands (the rim, the critical angle) are that file's, the slope-turn term of the critical band
taken over both meridians (the Frobenius norm of the sag's Hessian).  D and the worst deviation per case go to
profiles/biconic_accuracy.json.

The setter, the getter and the C parser need a context, which needs a device: tests/test_gpu_biconics.py covers them."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import asphere_ref as ar
import biconic_ref as br
from test_aspheres_cpu import _pkg, _lfo, COS_MIN, N_RAYS, ROOT

DATA = os.path.join(ROOT, "lens-flare_amd", "data")
EPS32 = float(np.finfo(np.float32).eps)
_cache = {}


def _lens():
    if "lens" not in _cache:
        _cache["lens"] = _pkg().load_lens_file("dgauss11_anamorphic.lens")
    return _cache["lens"]


def _f32(v):
    return float(np.float32(v))


def _cases():
    """the two curved cylinder faces of the shipped lens, and a general biconic: cx != cy, both non-zero, conics of opposite
    sign.  cx, cy are the float32 curvatures the library forms (1 / R in float)."""
    if "cases" in _cache:
        return _cache["cases"]
    lens = _lens()
    G = br.lens_geometry(lens)
    out = []
    for k in range(G["n"]):
        if G["bic_on"][k]:
            rx = np.float32(lens["biconics"]["radius_x"][k])
            out.append(dict(name=f"interface_{k}", cx=_f32(np.float32(1.0) / rx), cy=0.0, kx=0.0, ky=0.0, h=float(G["h"][k]),
                            n_before=1.0 if k == 0 else float(G["ior"][1][k - 1]), n_after=float(G["ior"][1][k])))
    out.append(dict(name="general", cx=_f32(np.float32(1.0) / np.float32(45.0)), cy=_f32(np.float32(1.0) / np.float32(30.0)),
                    kx=0.4, ky=-0.6, h=12.0, n_before=1.0, n_after=_f32(1.6)))
    _cache["cases"] = out
    return out


def _strong(s):
    return s["cx"] if abs(s["cx"]) >= abs(s["cy"]) else s["cy"]


def _dist(s):
    """how far in front of the vertex the rays start: test_aspheres_cpu._rays' 8 mm beyond the deepest point, over the disc
    of radius 1.1 h, of the surface and of the yardstick's sphere -- clear of either bowl (a cylinder of R = 77.5 is 12 mm
    deep at 1.1 x 38 mm)"""
    r = 1.1 * s["h"]
    z = [abs(float(br.sag(s["cx"], s["cy"], s["kx"], s["ky"], x, y)[0])) for x, y in ((r, 0.0), (0.0, r))]
    return 8.0 + max(z + [abs(float(ar.sag(_strong(s), 0.0, np.zeros(6), r * r)[0]))])


def _rays(s, forward, seed):
    """test_aspheres_cpu._rays with the origins' plane _dist(s) in front of the vertex: origins out to 1.1 h, aimed at points
    of the vertex plane out to 1.1 h -- every incidence up to grazing, hits out to the rim and past it.  float32 values."""
    rng = np.random.default_rng(seed)
    h = s["h"]
    def disc(rmax):
        r = rmax * np.sqrt(rng.random(N_RAYS)); a = 2 * np.pi * rng.random(N_RAYS)
        return r * np.cos(a), r * np.sin(a)
    ox, oy = disc(1.1 * h)
    tx, ty = disc(1.1 * h)
    z0 = -_dist(s) * (1.0 if forward else -1.0)
    v = np.stack([tx - ox, ty - oy, np.full(N_RAYS, -z0)], axis=1)
    d = (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)
    p = np.stack([ox, oy, np.full(N_RAYS, z0)], axis=1).astype(np.float32)
    return p, d, np.float32(z0)


def _D(s):
    """D as test_aspheres_cpu._yardstick measures it: the oracle's spherical float32 event against float64 (glass -> air: what
    geo_glass_event offers; the glass the interface's own), both directions of travel, refraction and reflection -- on the
    SAME rays as the biconic event gets, through the sphere of the stronger meridian's curvature"""
    key = ("D", s["name"])
    if key in _cache:
        return _cache[key]
    lfo = _lfo()
    D = 0.0
    c = _strong(s)
    eta = np.float32(max(s["n_before"], s["n_after"]))
    for forward in (0, 1):
        for reflect in (0, 1):
            p, d, z0 = _rays(s, forward, 10 + 2 * forward + reflect)
            ref = ar.event(p, d, 0.0, c, 0.0, np.zeros(6), s["h"], float(eta), 1.0, bool(reflect))
            for i in range(len(p)):
                st, pp, dd, w = lfo.geo_glass_event(p[i], d[i], 1.0, 0.0, c, np.float32(s["h"]) ** 2, eta, reflect, forward)
                if st != 0 or ref["fate"][i] != ar.ALIVE or ref["cos_i"][i] <= COS_MIN:
                    continue
                D = max(D, float(np.max(np.abs(pp - ref["p"][i]))), float(np.max(np.abs(dd - ref["d"][i]))))
    _cache[key] = D
    return D


def _critical_band(s, bar, n_in, n_out):
    """test_aspheres_cpu._critical_band with the slope's largest rate of change taken over both meridians"""
    turn = br.slope_turn(s["cx"], s["cy"], s["kx"], s["ky"], s["h"])
    eta2 = (n_in / n_out) ** 2
    return 2.0 * eta2 * turn * bar + 8.0 * EPS32 * max(1.0, eta2)


def _run(s, forward, reflect, seed, swap=False):
    """the float32 event and the float64 one on the rays of test_aspheres_cpu._rays"""
    pkg = _pkg()
    p, d, z0 = _rays(s, forward, seed)
    if swap:
        p = p[:, [1, 0, 2]].copy(); d = d[:, [1, 0, 2]].copy()
    n_in, n_out = (s["n_before"], s["n_after"]) if forward else (s["n_after"], s["n_before"])
    n_in32, n_out32 = np.float32(n_in), np.float32(n_out)
    rays = np.concatenate([p[:, :2], np.zeros((len(p), 1), np.float32), d * n_in32], axis=1).astype(np.float32)
    out, fates = pkg.biconic_event(s["cx"], s["cy"], s["kx"], s["ky"], s["h"], n_in32, n_out32, reflect, forward, z0, rays)
    ref = br.event(p, d, 0.0, s["cx"], s["cy"], s["kx"], s["ky"], s["h"], float(n_in32), float(n_out32), bool(reflect))
    n_leave = n_in32 if reflect else n_out32
    return dict(out=out, fates=fates, ref=ref, d32=out[:, 3:6].astype(np.float64) / float(n_leave), n_in=float(n_in32),
                n_out=float(n_out32), rays=rays, p=p, d=d, z0=z0)


def _bands(s, r, bar, reflect):
    """(clear, k, k_band): the rays float32 can decide -- float64 accepts them at cosine above 0.05, farther than the bar
    from the rim and (a refraction) farther than k_band from the critical angle"""
    ref = r["ref"]
    k = 1.0 - (r["n_in"] / r["n_out"]) ** 2 * (1.0 - ref["cos_i"] ** 2)
    k_band = _critical_band(s, bar, r["n_in"], r["n_out"])
    clear = (ref["fate"] == ar.ALIVE) & (ref["cos_i"] > COS_MIN) & (ref["rim"] > bar) & (bool(reflect) | (k > k_band))
    return clear, k, k_band


def test_the_analytic_slopes_agree_with_a_central_difference():
    for s in _cases():
        assert br.check_gradient(s["cx"], s["cy"], s["kx"], s["ky"], s["h"]) < 1e-8


def test_the_general_case_leaves_its_stronger_meridians_sphere_by_1000_bars():
    s = _cases()[-1]
    assert s["cx"] != s["cy"] and s["cx"] != 0 and s["cy"] != 0 and s["kx"] * s["ky"] < 0
    c = _strong(s)
    for x, y in ((s["h"], 0.0), (0.0, s["h"])):
        z = br.sag(s["cx"], s["cy"], s["kx"], s["ky"], x, y)[0]
        z0 = ar.sag(c, 0.0, np.zeros(6), s["h"] ** 2)[0]
        if abs(float(z - z0)) >= 1000 * 4 * _D(s):
            return
    raise AssertionError("the general biconic stays too near its sphere")


def test_the_event_against_float64_and_the_acceptance_rule():
    record = {}
    for s in _cases():
        D = _D(s)
        bar = 4 * D
        worst = 0.0
        counts = dict(rays=0, compared=0)
        for forward in (0, 1):
            for reflect in (0, 1):
                r = _run(s, forward, reflect, 10 + 2 * forward + reflect)
                ref, fates = r["ref"], r["fates"]
                clear, k, k_band = _bands(s, r, bar, reflect)
                counts["rays"] += len(fates); counts["compared"] += int(clear.sum())
                assert clear.sum() > 300                    # (leaving the glass most rays are totally reflected)
                # every ray float64 finds inside the aperture at incidence cosine above 0.05 is accepted ...
                assert np.all(fates[clear] == 0), (s["name"], forward, reflect, np.unique(fates[clear], return_counts=True))
                # ... no accepted ray is farther than the bar from the float64 hit (position and direction) ...
                both = (fates == 0) & (ref["fate"] == ar.ALIVE) & (ref["cos_i"] > COS_MIN)
                dev = np.maximum(np.max(np.abs(r["out"][both, 0:3] - ref["p"][both]), axis=1),
                                 np.max(np.abs(r["d32"][both] - ref["d"][both]), axis=1))
                worst = max(worst, float(dev.max()))
                # ... an accepted ray float64 rejects lies within the bar of the rim or of the critical angle ...
                odd = (fates == 0) & (ref["fate"] != ar.ALIVE) & (r["out"][:, 6] > COS_MIN * r["n_in"])
                assert np.all((ref["fate"][odd] != ar.MISSED)), "float32 accepts a ray that misses the surface in float64"
                assert np.all((ref["rim"][odd] <= bar) | (np.abs(k[odd]) <= k_band))
                # ... and what misses in float64 is dead in float32
                assert np.all(fates[ref["fate"] == ar.MISSED] != 0)
        print(f"{s['name']}: D = {D:.3e}, biconic event's worst deviation = {worst:.3e} ({worst / D:.2f} D)")
        record[s["name"]] = dict(cx=s["cx"], cy=s["cy"], kx=s["kx"], ky=s["ky"], D=D, bar=bar, biconic_worst=worst, **counts)
        assert worst <= bar, (s["name"], worst, bar)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "biconic_accuracy.json"), "w") as f:
        json.dump(dict(what="float32 event vs the float64 tracer of tests/biconic_ref.py on the two cylinder faces of "
                            "data/dgauss11_anamorphic.lens and a general biconic; D: the oracle's spherical event on the sphere "
                            "of the stronger meridian's curvature (existing code), biconic_worst: lf_biconic_event; mm and "
                            "unit-direction components, the larger of the two; the bar is 4 D",
                       rays_per_case=N_RAYS, cos_min=COS_MIN, **record), f, indent=1)
        f.write("\n")


def _compare_events(name, s, r, out2, fates2, bar, reflect):
    """two float32 events on the same rays: within the bar of each other where both live, equal fates outside the bands"""
    clear, k, k_band = _bands(s, r, bar, reflect)
    ref = r["ref"]
    assert clear.sum() > 300, name
    assert np.all(r["fates"][clear] == 0) and np.all(fates2[clear] == 0), name
    dev = np.abs(r["out"][clear, :6].astype(np.float64) - out2[clear, :6].astype(np.float64))
    assert dev.max() <= bar, (name, float(dev.max()), bar)
    decided = np.isfinite(ref["rim"]) & (ref["rim"] > bar) & (ref["cos_i"] > COS_MIN) & (bool(reflect) | (np.abs(k) > k_band))
    assert decided.sum() > clear.sum(), name           # (rays past the rim and totally reflected ones among them)
    # (fates as the march tells them apart: alive, vignetted -- missed or outside the aperture, one counter and one mask --
    # and totally reflected.  A grazing ray that lands millimetres PAST the rim may need more Newton steps than the count
    # that loses no accepted ray: the event with fewer steps calls it missed, the other outside the aperture, both dead.)
    merged = lambda f: np.where(f == 2, 1, f)
    assert np.array_equal(merged(r["fates"][decided]), merged(fates2[decided])), name
    missed = ref["fate"] == ar.MISSED
    assert np.all(r["fates"][missed] != 0) and np.all(fates2[missed] != 0), name
    return float(dev.max())


def test_degenerate_records_are_the_asphere_and_the_sphere():
    """1 / Rx = cy with kx = ky = kappa is lf_asphere_event's conicoid; with kappa = 0 it is the sphere of geo_glass_event"""
    pkg, lfo = _pkg(), _lfo()
    c, h = _f32(np.float32(1.0) / np.float32(30.0)), 12.0
    glass = _f32(1.6)
    for kappa in (-0.6, 0.4):
        s = dict(name=f"conicoid_{kappa}", cx=c, cy=c, kx=kappa, ky=kappa, h=h, n_before=1.0, n_after=glass)
        bar = 4 * _D(s)
        for forward in (0, 1):
            for reflect in (0, 1):
                r = _run(s, forward, reflect, 30 + 2 * forward + reflect)
                out2, fates2 = pkg.asphere_event(c, kappa, [], h, np.float32(r["n_in"]), np.float32(r["n_out"]), reflect, forward,
                                                 r["z0"], r["rays"])
                _compare_events(s["name"], s, r, out2, fates2, bar, reflect)
    s = dict(name="sphere", cx=c, cy=c, kx=0.0, ky=0.0, h=h, n_before=1.0, n_after=glass)
    bar = 4 * _D(s)
    for forward in (0, 1):           # (geo_glass_event: the ray arrives in the glass and leaves into air)
        for reflect in (0, 1):
            s_dir = dict(s, n_before=glass if forward else 1.0, n_after=1.0 if forward else glass)
            r = _run(s_dir, forward, reflect, 40 + 2 * forward + reflect)
            out2 = np.zeros((N_RAYS, 8), np.float32); fates2 = np.zeros(N_RAYS, np.int32)
            eta = np.float32(glass)
            for i in range(N_RAYS):
                st, pp, dd, w = lfo.geo_glass_event(r["p"][i], r["d"][i], 1.0, 0.0, c, np.float32(h) ** 2, eta, reflect, forward)
                fates2[i] = st
                n_leave = eta if reflect else np.float32(1.0)
                out2[i, 0:3] = pp; out2[i, 3:6] = np.asarray(dd, np.float32) * n_leave
            # (the oracle's statuses are not the event's fates: alive against dead is what the two share)
            r2 = dict(r, fates=(r["fates"] != 0).astype(np.int32))
            _compare_events("sphere", s_dir, r2, out2, (fates2 != 0).astype(np.int32), bar, reflect)


def test_transposition():
    """a record {1 / Rx = a} on base curvature b with rays (x, y) is the record {1 / Rx = b} on base a with rays (y, x), x and
    y swapped in the result: a swap of the meridians anywhere in the code cannot pass"""
    a, b = _f32(np.float32(1.0) / np.float32(45.0)), _f32(np.float32(1.0) / np.float32(-30.0))
    s1 = dict(name="transpose_ab", cx=a, cy=b, kx=0.4, ky=-0.6, h=12.0, n_before=1.0, n_after=_f32(1.6))
    s2 = dict(s1, name="transpose_ba", cx=b, cy=a, kx=-0.6, ky=0.4)
    bar = 4 * _D(s1)
    for forward in (0, 1):
        for reflect in (0, 1):
            r1 = _run(s1, forward, reflect, 60 + 2 * forward + reflect)
            r2 = _run(s2, forward, reflect, 60 + 2 * forward + reflect, swap=True)
            out2 = r2["out"][:, [1, 0, 2, 4, 3, 5, 6, 7]]
            worst = _compare_events("transposition", s1, r1, out2, r2["fates"], bar, reflect)
            assert np.any(r1["out"][r1["fates"] == 0, 0] != r1["out"][r1["fates"] == 0, 1])
    print(f"transposition: worst difference {worst:.3e}, bar {bar:.3e}")


def test_a_cylinder_leaves_the_other_meridian_alone():
    """cy = 0: K_y of every alive event is the K_y that entered, bit for bit; Rx = 0 on a curved row: the same for K_x"""
    cyl = _cases()[0]
    for s, comp in ((cyl, 4), (dict(cyl, name="cylinder_y", cx=0.0, cy=cyl["cx"]), 3)):
        n_alive = 0
        for forward in (0, 1):
            for reflect in (0, 1):
                r = _run(s, forward, reflect, 80 + 2 * forward + reflect)
                live = r["fates"] == 0
                n_alive += int(live.sum())
                assert np.array_equal(r["out"][live, comp].view(np.uint32), r["rays"][live, comp].view(np.uint32)), (s["name"], comp)
                other = 7 - comp
                if reflect == 0:
                    assert np.any(r["out"][live, other] != r["rays"][live, other])
        assert n_alive > 2000
    z, zx, zy = _pkg().biconic_sag(cyl["cx"], 0.0, 0.0, 0.0, 3.0, -7.0)
    assert zy == 0.0 and zx != 0.0
    z, zx, zy = _pkg().biconic_sag(0.0, cyl["cx"], 0.0, 0.0, 3.0, -7.0)
    assert zx == 0.0 and zy != 0.0


# ---- the shipped lens -----------------------------------------------------------------------------------------------------
def _paraxial(radius, lens, y, u, upto=None):
    """(height, slope) after the rows [0, upto) of the prescription at the middle wavelength: refraction, then transfer"""
    n1 = 1.0
    ior = np.asarray(lens["ior"], np.float64)[lens["ior"].shape[0] // 2]
    for k in range(lens["n"] if upto is None else upto):
        if k != lens["stop"]:
            c = 0.0 if radius[k] == 0 else 1.0 / float(radius[k])
            n2 = float(ior[k])
            u = c * (n1 - n2) / n2 * y + n1 / n2 * u
            n1 = n2
        y = y + float(lens["thickness"][k]) * u
    return y, u


def _scale(radius, lens):
    ys = [_paraxial(radius, lens, *yu, upto=lens["stop"])[0] for yu in ((1.0, 0.0), (0.0, 1.0))]
    y0 = -ys[1] / ys[0]
    return y0 * _paraxial(radius, lens, 1.0, 0.0)[0] + _paraxial(radius, lens, 0.0, 1.0)[0]


def _collimation(lens, xy):
    """rms spread (rad) of the directions the bundle of sensor point xy leaves the lens with, and the rays alive"""
    u = np.linspace(-0.9, 0.9, 13)
    uv = np.array([(a, b) for a in u for b in u])
    out = br.trace_path(lens, 1, -1, -1, np.tile(np.asarray(xy, np.float64), (len(uv), 1)), uv)[0]
    alive = out[:, 7] > 0
    # (the rms of a direction component, the larger of x and y: what test_aspheres_cpu asks of its lens's bundle)
    return float(max(out[alive, 3].std(), out[alive, 4].std())), int(alive.sum())


def test_the_shipped_lens_is_what_its_header_says():
    pkg = _pkg()
    lens = _lens()
    path = os.path.join(DATA, "dgauss11_anamorphic.lens")
    text = open(path).read()
    # the generator reproduces the file
    spec = importlib.util.spec_from_file_location("make_anamorphic_lens", os.path.join(DATA, "make_anamorphic_lens.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.generate(open(os.path.join(DATA, "dgauss11.lens")).read()) == text
    # dgauss11.lens behind four flat rows, two of them cylinders with power in x; three dispersive index columns
    base = pkg.load_lens_file("dgauss11.lens")
    assert lens["n"] == 15 and lens["stop"] == base["stop"] + 4
    for key in ("radius", "thickness", "semi_aperture"):
        assert np.array_equal(lens[key][4:], base[key])
    assert np.array_equal(lens["ior"][:, 4:], base["ior"]) and not lens["radius"][:4].any()
    b = lens["biconics"]
    assert list(np.nonzero(b["on"])[0]) == [1, 2] and np.all(b["radius_x"][[1, 2]] > 0) and not b["conic_x"].any() and not b["conic_y"].any()
    for k in (0, 2):
        assert lens["ior"][0, k] < lens["ior"][1, k] < lens["ior"][2, k]
    glass = [k for k in range(lens["n"]) if k != lens["stop"]]
    assert len(glass) * (len(glass) - 1) // 2 == 91
    # the two paraxial scales stand in the ratio the file states
    rx = np.where(b["on"] != 0, b["radius_x"], lens["radius"]).astype(np.float64)
    ry = lens["radius"].astype(np.float64)
    sx, sy = _scale(rx, lens), _scale(ry, lens)
    stated = float(re.search(r"squeeze \(scale_y / scale_x\) = ([0-9.]+)", text).group(1))
    assert abs(sy / sx - stated) < 2e-6 and stated > 1.3, (sx, sy, stated)
    # a unit-height collimated ray of either meridian meets the sensor within 1e-4 mm of the axis
    for r in (rx, ry):
        assert abs(_paraxial(r, lens, 1.0, 0.0)[0]) < 1e-4
    # the float64 tracer sends the bundles of the sensor centre and of one corner out collimated: under 2 mrad rms, where
    # dgauss11.lens itself stays under 1 mrad
    for xy in ((0.0, 0.0), (18.0, 12.0)):
        rms, n_alive = _collimation(lens, xy)
        rms0, n0 = _collimation(base, xy)
        print(f"sensor point {xy}: {rms * 1e3:.3f} mrad rms over {n_alive} rays; dgauss11.lens {rms0 * 1e3:.3f} mrad over {n0}")
        assert n_alive >= 10 and n0 >= 10
        assert rms < 2e-3 and rms0 < 1e-3


def test_the_python_parser_reads_biconic_lines(tmp_path):
    pkg = _pkg()
    src = open(os.path.join(DATA, "dgauss11.lens")).read()
    p = tmp_path / "ok.lens"
    p.write_text(src + "biconic 1 0\nbiconic 2 -55.5 0.25\nbiconic 8 30 -1 0.5\nasphere 3 -0.5 1e-6\n")
    lens = pkg.load_lens_file(str(p))
    b = lens["biconics"]
    assert b["on"].dtype == np.int32 and list(np.nonzero(b["on"])[0]) == [1, 2, 8]
    assert np.array_equal(b["radius_x"][[1, 2, 8]], np.array([0, -55.5, 30], np.float32))
    assert np.array_equal(b["conic_x"][[1, 2, 8]], np.array([0, 0.25, -1], np.float32))
    assert np.array_equal(b["conic_y"][[1, 2, 8]], np.array([0, 0, 0.5], np.float32))
    assert "biconics" not in pkg.load_lens_file("dgauss11.lens") and lens["aspheres"]["conic"][3] == np.float32(-0.5)
    # the lines round-trip: written back from the parsed arrays, the file parses to the same arrays
    q = tmp_path / "again.lens"
    q.write_text(src + "".join(f"biconic {k} {float(b['radius_x'][k])!r} {float(b['conic_x'][k])!r} {float(b['conic_y'][k])!r}\n" for k in np.nonzero(b["on"])[0]))
    b2 = pkg.load_lens_file(str(q))["biconics"]
    for key in b:
        assert np.array_equal(b[key], b2[key])
    for bad in ("biconic 5 40\n",                        # the stop
                "asphere 2 -0.5\nbiconic 2 40\n",        # an interface with an asphere line
                "biconic 2\n", "biconic 2 40 0 0 0\n", "biconic 2 forty\n",     # malformed
                "biconic 11 40\n", "biconic -1 40\n",    # out of range
                "biconic 2 40\nbiconic 2 40\n"):
        p = tmp_path / "bad.lens"
        p.write_text(src + bad)
        with pytest.raises(ValueError):
            pkg.load_lens_file(str(p))
