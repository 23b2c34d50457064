"""Ghost occlusion for point lights without a device (lf_set_ghost_occlusion_reach): the four entry points are declared and
exported, the Python wrappers refuse bad arguments before they reach the library, lf_ghost_shadow_reach -- the
`__host__ __device__` definition the occlusion kernels call (lens-flare_amd/csrc/lf_march_events.h lf_point_shadow_reach) --
is the float64 expression, and the frame plan is where it was.  What the march does with it is tests/test_gpu_near_occlusion.py's.

THE BAR on |t - t64|, derived, not fitted.  t = wpm ((s.x dc.x + s.y dc.y) + s.z dc.z) with s = L - P and dc = d (1 / |d|),
all in double on float32 inputs: three subtractions, |d|^2 (five roundings), a root, a division, three products by 1 / |d|,
three products, two sums and the product by wpm -- fewer than 16 roundings of at most 2^-53 relative each, every one on a
term bounded by |s| (|dc| <= 1 + a few ulp).  numpy's float64 runs the same expression and may round any of them the other
way: |t - t64| <= 16 * 2^-52 * wpm * |s|."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_near_lights_cpu import exit_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lens-flare_amd", "host")
DIRECTIONAL, POINT = 0, 1
N = 4096
CTX_SYMBOLS = ["lf_set_ghost_occlusion_reach", "lf_get_ghost_occlusion_reach", "lf_ghost_ray_light_visibility"]
HOST_SYMBOL = "lf_ghost_shadow_reach"
# lamps at 90 mm, 300 mm, 1 m and 10 km, the lobes the rays are drawn around, the scales
LAMPS = [(1.5, -1.0, -90.0), (-3.0, 2.0, -300.0), (20.0, -12.0, -1000.0), (4.0e4, -3.0e4, -1.0e7)]
ALPHAS = (0.05, 0.03, 0.1, 0.02)
WPMS = (1e-3, 1.0, 2.5e-2)
ZV = 12.5        # the front vertex of the cap the exit points lie on: the rays carry z absolute, front vertex + sag


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def _rays(k):
    """N seeded exit rays on the front cap, z absolute, each within 1.6 lobe radii of lamp k as seen from its own exit point"""
    rng = np.random.default_rng(0x0CC1 + k)
    lamp = np.asarray(LAMPS[k], np.float64) - [0.0, 0.0, ZV]
    r = exit_rays(rng, N, lamp, POINT, ALPHAS[k]).astype(np.float64)
    r[:, 2] += ZV
    return r.astype(np.float32)


def reach64(L32, rays32, wpm, px=1.0, py=1.0, pz=1.0, z_off=0.0, sx=1.0, sy=1.0, scale=True):
    """the contract's expression in numpy float64 on the float32 inputs; the keyword arguments are the mutants"""
    r = np.asarray(rays32, np.float32).astype(np.float64)
    L = np.asarray(L32, np.float32).astype(np.float64)
    s = np.stack([sx * (L[0] - px * r[:, 0]), sy * (L[1] - py * r[:, 1]), L[2] - pz * (r[:, 2] - z_off)], 1)
    d = r[:, 3:]
    rn = 1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    dc = d * rn[:, None]
    t = (wpm if scale else 1.0) * ((s[:, 0] * dc[:, 0] + s[:, 1] * dc[:, 1]) + s[:, 2] * dc[:, 2])
    return np.where(t > 0.0, t, 0.0), np.linalg.norm(s, axis=1)


def test_the_four_symbols_are_declared_and_exported():
    pkg = _pkg()
    header = open(os.path.join(ROOT, "include", "lensflare.h")).read()
    lib = pkg.load_library()
    for s in CTX_SYMBOLS:
        assert re.search(r"lf_status\s+%s\s*\(\s*lf_ctx\s*\*" % s, header), s
        assert s in pkg.ABI_SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s)(*([C.c_void_p(0)] * 6)) == 1, s      # a NULL context: LF_ERR_INVALID, nothing dereferenced
    # the host function takes no context: NULL vectors are LF_ERR_INVALID as well
    assert re.search(r"^lf_status\s+%s\s*\(\s*int kind,\s*const float vec\[3\],\s*const float ray\[6\],\s*double world_per_mm,\s*"
                     r"double\s*\*\s*reach\)" % HOST_SYMBOL, header, re.M)
    assert HOST_SYMBOL in pkg.ABI_SYMBOLS and hasattr(lib, HOST_SYMBOL)
    assert getattr(lib, HOST_SYMBOL)(C.c_int(POINT), C.c_void_p(0), C.c_void_p(0), C.c_double(1e-3), C.c_void_p(0)) == 1
    assert "typedef enum { LF_OCCLUSION_REACH_SKY = 0, LF_OCCLUSION_REACH_LIGHT = 1 } lf_occlusion_reach;" in header
    assert (pkg.OCCLUSION_REACH_SKY, pkg.OCCLUSION_REACH_LIGHT) == (0, 1)
    for name in ("set_ghost_occlusion_reach", "get_ghost_occlusion_reach", "ghost_ray_light_visibility"):
        assert callable(getattr(pkg.LensFlare, name)), name
    assert callable(pkg.ghost_shadow_reach)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper reached the library ({name}) with arguments it should have refused")


def _bare(pkg):
    """a wrapper object with no context and no library behind it: whatever reaches the library fails the test"""
    lf = pkg.LensFlare.__new__(pkg.LensFlare)
    lf.lib, lf.ctx, lf._owned = _NoLibrary(), C.c_void_p(), False
    return lf


def test_the_wrappers_validate_their_arguments_without_a_device(monkeypatch):
    pkg = _pkg()
    lf = _bare(pkg)
    for bad in (2, -1, 1.0, "light", None, True):
        with pytest.raises(ValueError):
            lf.set_ghost_occlusion_reach(bad)
    for rays in (np.zeros(6), np.zeros((4, 5)), np.zeros((2, 3, 6)), [[0, 0, 0, 0, 0, 0.0]], [[0, 0, float("nan"), 0, 0, -1.0]],
                 [[float("inf"), 0, 0, 0, 0, -1.0]]):
        with pytest.raises(ValueError):
            lf.ghost_ray_light_visibility(rays)
    # ... and what is fine does reach it
    for good in (pkg.OCCLUSION_REACH_SKY, pkg.OCCLUSION_REACH_LIGHT):
        with pytest.raises(AssertionError):
            lf.set_ghost_occlusion_reach(good)
    with pytest.raises(AssertionError):
        lf.get_ghost_occlusion_reach()
    with pytest.raises(AssertionError):
        lf.ghost_ray_light_visibility([[0, 0, 0, 0, 0, -1.0]])
    # the module-level host function
    monkeypatch.setattr(pkg, "load_library", lambda: _NoLibrary())
    ray = [[0.0, 0.0, 0.0, 0.0, 0.0, -1.0]]
    for kind, vec, rays, wpm in ((2, LAMPS[0], ray, 1e-3), (-1, LAMPS[0], ray, 1e-3), (POINT, [0.0, 1.0], ray, 1e-3),
                                 (POINT, [0.0, float("nan"), -90.0], ray, 1e-3), (POINT, LAMPS[0], np.zeros(6), 1e-3),
                                 (POINT, LAMPS[0], np.zeros((3, 5)), 1e-3), (POINT, LAMPS[0], [[0, 0, 0, 0, 0, 0.0]], 1e-3),
                                 (POINT, LAMPS[0], [[0, float("inf"), 0, 0, 0, -1.0]], 1e-3), (POINT, LAMPS[0], ray, 0.0),
                                 (POINT, LAMPS[0], ray, -1e-3), (POINT, LAMPS[0], ray, float("nan")),
                                 (DIRECTIONAL, LAMPS[0], ray, float("inf"))):
        with pytest.raises(ValueError):
            pkg.ghost_shadow_reach(kind, vec, rays, wpm)
    with pytest.raises(AssertionError):
        pkg.ghost_shadow_reach(POINT, LAMPS[0], ray, 1e-3)


def test_the_library_refuses_what_the_wrapper_refuses():
    """lf_ghost_shadow_reach itself: a bad kind, a scale that is not finite or <= 0, a non-finite input -- LF_ERR_INVALID"""
    lib = _pkg().load_library()
    fp = lambda a: np.asarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    out = C.c_double(-1.0)
    ok_v, ok_r = np.asarray(LAMPS[0], np.float32), np.asarray([0, 0, 0, 0, 0, -1.0], np.float32)
    call = lambda kind, v, r, w: lib.lf_ghost_shadow_reach(C.c_int(kind), fp(v), fp(r), C.c_double(w), C.byref(out))
    assert call(POINT, ok_v, ok_r, 1e-3) == 0 and out.value == pytest.approx(0.09, rel=1e-6)
    for kind, v, r, w in ((2, ok_v, ok_r, 1e-3), (POINT, ok_v, ok_r, 0.0), (POINT, ok_v, ok_r, -1.0), (POINT, ok_v, ok_r, float("inf")),
                          (POINT, ok_v, ok_r, float("nan")), (POINT, [0, float("nan"), -90.0], ok_r, 1e-3),
                          (DIRECTIONAL, ok_v, [0, 0, float("inf"), 0, 0, -1.0], 1e-3)):
        assert call(kind, np.asarray(v, np.float32), np.asarray(r, np.float32), w) == 1, (kind, v, r, w)


def test_shadow_reach_is_the_float64_expression_within_the_derived_bar():
    pkg = _pkg()
    for k, lamp in enumerate(LAMPS):
        rays = _rays(k)
        L32 = np.asarray(lamp, np.float32)
        for wpm in WPMS:
            t = pkg.ghost_shadow_reach(POINT, lamp, rays, wpm)
            t64, s_len = reach64(L32, rays, wpm)
            bar = 16.0 * 2.0 ** -52 * wpm * s_len
            err = np.abs(t - t64)
            assert (err <= bar).all(), (k, wpm, float((err / bar).max()))
            assert (t > 0.0).all() and np.isfinite(t).all()
            # ... the point of the ray nearest the lamp: within the lobe's spread |s| cos(1.6 alpha) <= t / wpm <= |s|
            assert (t <= wpm * s_len * (1.0 + 1e-6)).all() and (t >= wpm * s_len * np.cos(1.7 * ALPHAS[k])).all()
            # the mutants: each misses the bar on (nearly) every ray -- the exit point dropped, z without the front vertex's
            # offset, x or y flipped, the scale omitted
            mutants = dict(no_exit_point=dict(px=0.0, py=0.0, pz=0.0), z_relative=dict(z_off=ZV), x_flipped=dict(sx=-1.0),
                           y_flipped=dict(sy=-1.0))
            if wpm != 1.0:
                mutants["no_scale"] = dict(scale=False)
            for name, kw in mutants.items():
                tm, _ = reach64(L32, rays, wpm, **kw)
                assert (np.abs(t - tm) > bar).mean() > 0.9, (k, wpm, name)
            # a directional light reaches the sky, whatever the ray
            assert np.array_equal(pkg.ghost_shadow_reach(DIRECTIONAL, lamp, rays[:64], wpm), np.full(64, np.inf))
            # a ray that looks away from the lamp: exactly 0
            away = rays.copy()
            away[:, 3:] = -(L32.astype(np.float64)[None, :] - rays[:, :3].astype(np.float64)).astype(np.float32)
            ta = pkg.ghost_shadow_reach(POINT, lamp, away, wpm)
            assert np.array_equal(ta, np.zeros(N)) and not np.signbit(ta).any()


def test_the_frame_plan_is_where_it_was_and_does_not_carry_the_reach():
    """the setting is the context's: lf_frame_sequence.h installs occlusion as it did and never the reach; the mirrors' plans
    are filled as they were, and the stand-alone mirror sets the reach on its context directly"""
    seq = open(os.path.join(HOST, "lf_frame_sequence.h")).read()
    assert re.search(r"lf_set_ghost_occlusion\(ctx, \(p->ghost_occlusion && p->ghosts == LF_FRAME_GHOSTS_MARCH\) \? 1 : 0,\s*p->world_per_mm\)", seq)
    assert "lf_set_ghost_occlusion_reach" not in seq and "reach" not in seq
    assert re.search(r"int ghost_occlusion;[^}]*\}\s*lf_frame_plan;", seq, re.S)
    assert not re.search(r"int ghost_occlusion;[^}]*;[^}]*\}\s*lf_frame_plan;", seq, re.S)      # the last member
    dropin = open(os.path.join(HOST, "pathtracer_amd.cpp")).read()
    assert re.findall(r"plan\.ghost_occlusion\s*=\s*([^;]+);", dropin) == ["0"]
    assert "lf_set_ghost_occlusion_reach" not in dropin
    mirror = open(os.path.join(HOST, "lf_pathtracer.cpp")).read()
    assert re.findall(r"plan\.ghost_occlusion\s*=\s*([^;]+);", mirror) == ["ghost_occlusion_ ? 1 : 0"]
    assert re.search(r"void PathTracer::use_ghost_occlusion_reach\(int reach\)\s*\{\s*check\(lf_set_ghost_occlusion_reach\(ctx_, reach\)", mirror)
    assert re.search(r"void use_ghost_occlusion_reach\(int reach\);", open(os.path.join(HOST, "lf_pathtracer.h")).read())
    demo = open(os.path.join(HOST, "shim_demo.cpp")).read()
    assert "geolamp" in demo and "use_ghost_occlusion_reach(LF_OCCLUSION_REACH_LIGHT)" in demo
