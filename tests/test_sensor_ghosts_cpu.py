"""Sensor-reflection ghosts, the host side (lf_set_sensor_ghosts; lens-flare_amd/csrc/lf_sensor_event.h, lf_march_sensor.hip): the
path's order against Python, the mirror event against float64, the lens file's new line, the symbols, and the float64
tracer's own side of the exclusions the GPU comparison uses (tests/test_gpu_sensor_ghosts.py).  No GPU.  (The C parser needs a
context: its cases are in the GPU file, as the aspheres' are.)"""
import ctypes as C
import os

import numpy as np
import pytest

import asphere_ref as ar
import sensor_ghost_ref as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LF_ERR_INVALID = 1
W, H = 128, 64
D_STANDIN = 2.6e-5          # the event yardstick's size (tests/test_aspheres_cpu.py _yardstick); the GPU test measures it
COS_MIN = 0.05
# sensor paths of a recorded lens that would take the exclusions past 2 % of its grid: named here, dropped from the GPU
# comparison of that lens (dgauss11.lens keeps every path)
OVER_CAP = {"dgauss11.lens": (), "dgauss11_asph.lens": (), "dgauss11_anamorphic.lens": ()}
_cache = {}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def interfaces(lens):
    return [k for k in range(int(lens["n"])) if k != int(lens["stop"])]


def traced(pkg, name, lam=1):
    """the float64 tracer over the fixed grid for every sensor path of lens file `name`, bare and with dgauss11_coated.lens's
    films in ONE trace (the bare weight rides along), under an OPEN stop (no mask: the housing alone clips), once per session:
    {i: trace_sensor_path's tuple}"""
    if name not in _cache:
        lens = pkg.load_lens_file(name)
        xy, uv = ar.comparison_grid()
        hw, hh = sg.rectangle(W, H, lens["sensor_width_mm"])
        coat = pkg.load_lens_file("dgauss11_coated.lens")["coatings"]
        if len(coat["thickness_nm"]) != int(lens["n"]):       # (the anamorphic lens has interfaces of its own: traced bare)
            coat = None
        _cache[name] = dict(lens=lens, xy=xy, uv=uv, coat=coat, half=(hw, hh),
                            paths={i: sg.trace_sensor_path(lens, lam, i, xy, uv, hw, hh, 1.0, None, coat) for i in interfaces(lens)})
    return _cache[name]


# ---- 1. the order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,stop", [(11, 5), (16, 7)])
def test_the_sequence_is_pythons(pkg, n, stop):
    lib = pkg.load_library()
    for i in range(n):
        if i == stop:
            continue
        got = pkg.sensor_path_sequence(n, stop, i)
        assert len(got) == 3 * n - 2 * i
        assert np.array_equal(got, sg.coded(n, i)), i
        assert np.count_nonzero(got == (n | 1 << 8 | 1 << 9)) == 1
    out = np.zeros(64, np.int32); n_ev = C.c_int()
    call = lambda i, cap: lib.lf_sensor_path_sequence(n, stop, i, out.ctypes.data_as(C.POINTER(C.c_int)), cap, C.byref(n_ev))
    assert call(0, 3 * n) == 0 and n_ev.value == 3 * n
    assert call(stop, 64) == LF_ERR_INVALID
    assert call(-1, 64) == LF_ERR_INVALID and call(n, 64) == LF_ERR_INVALID
    assert call(0, 3 * n - 1) == LF_ERR_INVALID
    assert call(n - 1, n + 2) == 0 and call(n - 1, n + 1) == LF_ERR_INVALID


# ---- 2. the event ---------------------------------------------------------------------------------------------------------
def test_the_mirror_event_against_float64(pkg):
    """1000 rays from points behind a rear element (|x|, |y| up to 12 mm, z up to 4 mm off its vertex) towards a plane 36 mm on,
    slopes up to 0.6: the hit and the mirrored direction against float64 on the same float32 inputs.  The bar is the float32
    spacing of what the transfer forms, as lf_asphere.h's criterion counts it (eps = 2^-24, half a spacing per rounding):
    t = -(z + dzv) / K_z carries the sum's and the quotient's rounding, 2 eps |t|; x = fma(t, K_x, p_x) moves by that times
    |K_x| and rounds once more, eps (|t K_x| + |p_x|) -- 3 eps (|t K_x| + |p_x|) covers both, likewise y.  The direction is
    copied, K_z negated: exact.  Inside / lost must agree wherever float64 lands farther than that bar from an edge."""
    rng = np.random.default_rng(11)
    n = 1000
    dzv = np.float32(-36.106)
    rays = np.zeros((n, 6), np.float32)
    rays[:, 0:2] = rng.uniform(-12, 12, (n, 2)); rays[:, 2] = rng.uniform(-4, 4, n)
    rays[:, 3:5] = rng.uniform(-0.6, 0.6, (n, 2)); rays[:, 5] = rng.uniform(0.7, 1.7, n)
    hw, hh = np.float32(18.0), np.float32(9.0)
    out, inside = pkg.sensor_mirror_event(rays, dzv, hw, hh)
    r = rays.astype(np.float64)
    t = -(r[:, 2] + float(dzv)) / r[:, 5]
    x = r[:, 0] + t * r[:, 3]; y = r[:, 1] + t * r[:, 4]
    eps = 2.0 ** -24
    bx = 3 * eps * (np.abs(t * r[:, 3]) + np.abs(r[:, 0])); by = 3 * eps * (np.abs(t * r[:, 4]) + np.abs(r[:, 1]))
    assert np.all(np.abs(out[:, 0] - x) <= bx) and np.all(np.abs(out[:, 1] - y) <= by)
    assert np.all(out[:, 2] == 0)
    assert np.array_equal(out[:, 3:5], rays[:, 3:5]) and np.array_equal(out[:, 5], -rays[:, 5])
    want = (np.abs(x) <= float(hw)) & (np.abs(y) <= float(hh))
    clear = (np.abs(np.abs(x) - float(hw)) > bx) & (np.abs(np.abs(y) - float(hh)) > by)
    assert clear.sum() > 990 and 100 < want.sum() < 900          # (both fates, and the edge band is thin)
    assert np.array_equal(inside[clear] == 1, want[clear])
    # a ray parallel to the plane, a NaN: lost, never inside
    odd = np.array([[1, 1, 0, 0.1, 0.1, 0.0], [np.nan, 0, 0, 0, 0, 1.0]], np.float32)
    assert not pkg.sensor_mirror_event(odd, dzv, hw, hh)[1].any()


# ---- 3. the lens file -----------------------------------------------------------------------------------------------------
def test_the_python_parser_reads_the_line(pkg, tmp_path):
    shipped = pkg.load_lens_file("dgauss11_sensor.lens")
    plain = pkg.load_lens_file("dgauss11.lens")
    assert np.array_equal(shipped["sensor_reflectance"], np.full(3, 0.05, np.float32))
    assert "sensor_reflectance" not in plain
    for key in ("radius", "thickness", "ior", "semi_aperture"):
        assert np.array_equal(shipped[key], plain[key])
    body = open(os.path.join(ROOT, "lens-flare_amd", "data", "dgauss11.lens")).read()
    def load(line):
        p = tmp_path / "t.lens"
        p.write_text(body + line + "\n")
        return pkg.load_lens_file(str(p))
    assert np.array_equal(load("sensor_reflectance 0.02 0.04 0.08")["sensor_reflectance"], np.array([0.02, 0.04, 0.08], np.float32))
    assert np.array_equal(load("sensor_reflectance 0.25")["sensor_reflectance"], np.full(3, 0.25, np.float32))
    for bad in ("sensor_reflectance", "sensor_reflectance 0.1 0.2", "sensor_reflectance 1.5", "sensor_reflectance -0.1 0 0",
                "sensor_reflectance 0.1\nsensor_reflectance 0.1", "sensor_reflectance x"):
        with pytest.raises(ValueError):
            load(bad)


# ---- 4. symbols -----------------------------------------------------------------------------------------------------------
def test_symbols_refusals_and_methods(pkg):
    lib = pkg.load_library()
    names = ("lf_set_sensor_reflectance", "lf_get_sensor_reflectance", "lf_set_sensor_ghosts", "lf_get_sensor_ghosts",
             "lf_march_sensor_path_rays", "lf_sensor_path_sequence", "lf_sensor_mirror_event", "lf_get_sensor_ghost_stats")
    for s in names:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS, s
    assert "lf_" + "get_sensor_ghost_stats" in open(os.path.join(ROOT, "include", "lensflare.h")).read()
    f4 = (C.c_float * 4)(); i4 = (C.c_int * 4)(); u4 = (C.c_uint64 * 4)(); one = C.c_int()
    assert lib.lf_set_sensor_reflectance(None, 3, f4) == LF_ERR_INVALID
    assert lib.lf_get_sensor_reflectance(None, 3, f4, C.byref(one)) == LF_ERR_INVALID
    assert lib.lf_set_sensor_ghosts(None, 1, None, 0) == LF_ERR_INVALID
    assert lib.lf_get_sensor_ghosts(None, C.byref(one), i4, 4, C.byref(one)) == LF_ERR_INVALID
    assert lib.lf_march_sensor_path_rays(None, 0, 0, C.c_size_t(1), f4, f4, f4) == LF_ERR_INVALID
    assert lib.lf_get_sensor_ghost_stats(None, u4) == LF_ERR_INVALID
    assert lib.lf_sensor_mirror_event(None, C.c_float(0), C.c_float(1), C.c_float(1), f4, C.byref(one)) == LF_ERR_INVALID
    for m in ("set_sensor_reflectance", "sensor_reflectance", "set_sensor_ghosts", "sensor_ghosts", "march_sensor_path_rays",
              "sensor_path_sequence", "sensor_ghost_stats"):
        assert callable(getattr(pkg.LensFlare, m)), m
    assert (pkg.SENSOR_GHOSTS_OFF, pkg.SENSOR_GHOSTS_ADD, pkg.SENSOR_GHOSTS_ONLY) == (0, 1, 2)


# ---- 5. the cap -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dgauss11.lens", "dgauss11_asph.lens", "dgauss11_anamorphic.lens"])
def test_the_tracers_side_of_the_exclusions(pkg, name):
    """Over the 588-ray grid, column 1, the rectangle of a 128 x 64 frame on 36 mm: a ray is left out if the tracer finds it
    within 4 D (3 n - 2 i) mm of an aperture rim or of the rectangle's edge, or at an incidence cosine <= 0.05.  At most 2 %
    of all (path, ray) cases are left out (and of every path that the GPU comparison keeps); the tracer brings at least 300
    rays out alive, at least 5 on every path."""
    T = traced(pkg, name)
    n = int(T["lens"]["n"])
    per_path, left_by_path = {}, {}
    for i, t in T["paths"].items():
        out, cmin, rim, done, wb, edge = t
        skip = sg.excluded(cmin, rim, edge, 4 * D_STANDIN * (3 * n - 2 * i), COS_MIN)
        left_by_path[i] = int(skip.sum())
        per_path[i] = int((out[:, 7] == 1).sum())
        assert np.all(np.isfinite(out[out[:, 7] == 1]))
    kept = [i for i in T["paths"] if i not in OVER_CAP[name]]
    total, left = len(T["xy"]) * len(kept), sum(left_by_path[i] for i in kept)
    alive = sum(per_path[i] for i in kept)
    print(f"{name}: left out {left} of {total} (per path {left_by_path}); alive {alive} (per path {per_path}); dropped {OVER_CAP[name]}")
    assert left <= 0.02 * total
    assert alive >= 300 and min(per_path[i] for i in kept) >= 5, per_path
