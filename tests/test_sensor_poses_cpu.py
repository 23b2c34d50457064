"""Sensor ghosts through decentred and tilted lenses, the host side (lf_set_sensor_ghost_surfaces; lens-flare_amd/csrc/
lf_march_sensor.hip): the symbols and bindings, and the float64 tracer of tests/sensor_pose_ref.py on its own -- it equals the
centred tracer on a lens without records, its side of the exclusions the GPU comparison uses stays under the cap, and the
poses of the shipped lens move its exit rays by many bars (so a kernel that ignored the records cannot pass
tests/test_gpu_sensor_poses.py).  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import asphere_ref as ar
import sensor_ghost_ref as sg
import sensor_pose_ref as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LF_ERR_INVALID = 1
W, H = 128, 64
D_STANDIN = 2.6e-5          # the event yardstick's size (tests/test_aspheres_cpu.py _yardstick); the GPU test measures it
COS_MIN = 0.05
POSED = "dgauss11_decentred.lens"
_cache = {}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def interfaces(lens):
    return [k for k in range(int(lens["n"])) if k != int(lens["stop"])]


def traced(pkg, lens, key, lam=1):
    """sensor_pose_ref.trace_sensor_path over the fixed grid for every sensor path of `lens` (a parsed lens; `key` names it in
    the cache), bare and with dgauss11_coated.lens's films in ONE trace (the bare weight rides along), under an OPEN stop,
    once per session: {i: the tracer's tuple}"""
    if key not in _cache:
        xy, uv = ar.comparison_grid()
        hw, hh = sg.rectangle(W, H, lens["sensor_width_mm"])
        coat = pkg.load_lens_file("dgauss11_coated.lens")["coatings"]
        _cache[key] = dict(lens=lens, xy=xy, uv=uv, coat=coat, half=(hw, hh),
                           paths={i: sp.trace_sensor_path(lens, lam, i, xy, uv, hw, hh, 1.0, None, coat) for i in interfaces(lens)})
    return _cache[key]


def cleared(lens):
    """the same prescription with its pose records cleared"""
    out = dict(lens)
    out.pop("poses", None)
    return out


# ---- 1. symbols and bindings ----------------------------------------------------------------------------------------------
def test_symbols_and_bindings(pkg):
    lib = pkg.load_library()
    for s in ("lf_set_sensor_ghost_surfaces", "lf_get_sensor_ghost_surfaces"):
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS, s
        assert s in open(os.path.join(ROOT, "include", "lensflare.h")).read()
    one = C.c_int()
    assert lib.lf_set_sensor_ghost_surfaces(None, 1) == LF_ERR_INVALID
    assert lib.lf_set_sensor_ghost_surfaces(None, 0) == LF_ERR_INVALID
    assert lib.lf_get_sensor_ghost_surfaces(None, C.byref(one)) == LF_ERR_INVALID
    assert (pkg.SENSOR_SURFACES_CENTRED, pkg.SENSOR_SURFACES_POSED) == (0, 1)
    for m in ("set_sensor_ghost_surfaces", "sensor_ghost_surfaces"):
        assert callable(getattr(pkg.LensFlare, m)), m


# ---- 2. the un-posed case -------------------------------------------------------------------------------------------------
def test_without_records_the_tracer_is_the_centred_one(pkg):
    lens = pkg.load_lens_file("dgauss11.lens")
    xy, uv = ar.comparison_grid()
    hw, hh = sg.rectangle(W, H, lens["sensor_width_mm"])
    for i in interfaces(lens):
        a = sg.trace_sensor_path(lens, 1, i, xy, uv, hw, hh, 0.5)
        b = sp.trace_sensor_path(lens, 1, i, xy, uv, hw, hh, 0.5)
        assert len(b) == len(a) + 1 and np.all(np.isinf(b[6]))          # (no posed row was met)
        assert np.array_equal(a[0][:, 7], b[0][:, 7]) and np.array_equal(a[3], b[3]), i
        live = a[0][:, 7] == 1
        assert np.max(np.abs(a[0][live] - b[0][live]), initial=0.0) <= 1e-9, i
        for x, y in zip(a[1:], b[1:6]):
            fin = np.isfinite(x)
            assert np.array_equal(fin, np.isfinite(y)) and np.max(np.abs(x[fin] - y[fin]), initial=0.0) <= 1e-9, i


# ---- 3. the cap -----------------------------------------------------------------------------------------------------------
def test_the_tracers_side_of_the_exclusions(pkg):
    """dgauss11_decentred.lens, column 1, an open stop, the rectangle of a 128 x 64 frame, every interface but the stop: a ray
    is left out if the tracer finds it within 4 D (3 n - 2 i) mm of an aperture rim or of the rectangle's edge, at an
    incidence cosine <= 0.05, or with a towards_margin <= that bar.  At most 2 % of all (path, ray) cases are left out; at
    least 300 rays come out alive, at least 5 on every path.  (Measured with D = 2.6e-5: 54 of 5880 left out, 355 alive, 7 on
    the poorest path.)"""
    T = traced(pkg, pkg.load_lens_file(POSED), POSED)
    n = int(T["lens"]["n"])
    per_path, left_by_path = {}, {}
    for i, t in T["paths"].items():
        out, cmin, rim, done, wb, edge, towards = t
        skip = sp.left_out(cmin, rim, edge, towards, 4 * D_STANDIN * (3 * n - 2 * i), COS_MIN)
        left_by_path[i] = int(skip.sum())
        per_path[i] = int((out[:, 7] == 1).sum())
        assert np.all(np.isfinite(out[out[:, 7] == 1]))
    total, left = len(T["xy"]) * len(T["paths"]), sum(left_by_path.values())
    alive = sum(per_path.values())
    print(f"{POSED}: left out {left} of {total} (per path {left_by_path}); alive {alive} (per path {per_path})")
    assert len(T["paths"]) == n - 1
    assert left <= 0.02 * total
    assert alive >= 300 and min(per_path.values()) >= 5, per_path


# ---- 4. the poses are visible ---------------------------------------------------------------------------------------------
def test_the_poses_move_the_exit_rays_by_many_bars(pkg):
    """the shipped lens against the same prescription with its poses cleared, on the rays alive in both: on every path the
    exit point moves by at least ten bars (4 D n_ev) somewhere on the grid"""
    lens = pkg.load_lens_file(POSED)
    A = traced(pkg, lens, POSED)
    B = traced(pkg, cleared(lens), POSED + " cleared")
    n = int(lens["n"])
    seen = {}
    for i in A["paths"]:
        a, b = A["paths"][i][0], B["paths"][i][0]
        both = (a[:, 7] == 1) & (b[:, 7] == 1)
        assert both.sum() >= 5, i
        bar = 4 * D_STANDIN * (3 * n - 2 * i)
        seen[i] = (float(np.max(np.abs(a[both, 0:3] - b[both, 0:3]))), bar)
        assert np.all(np.isinf(B["paths"][i][6]))
    print("exit point moved by / the bar (mm), per path:", {i: (round(v, 4), round(b, 5)) for i, (v, b) in seen.items()})
    for i, (v, bar) in seen.items():
        assert v >= 10 * bar, (i, v, bar)
