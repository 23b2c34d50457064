"""Multi-layer anti-reflection stacks, host side (no device): lf_coating_stack_reflectance -- the march's float32 stack
arithmetic (lf_march_events.h stack_fraction, the recursive Airy form) evaluated on the host -- against an independent
float64 characteristic-matrix (Abeles) formula written here from the textbook, its closed forms, its equivalences with
the single film, and the `layer` lines of the lens-file syntax."""
import math
import os
import re

import numpy as np
import pytest

from test_coatings_cpu import airy64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS = (656.3, 587.6, 486.1)
FILMS = (1.38, 1.46, 1.63, 2.05, 2.3)
# The bars start from the single film's (coated_fraction: |dR| <= 5.3e-7 away from the critical angle, relative <= 6.1e-6
# on the transmitted fraction 1 - R).  stack_fraction keeps the relative one (worst measured on the grid below: 1.27e-6)
# and misses the absolute one: worst |dR| = 6.62e-7 against the matrix formula -- up to six float32 phases of several turns
# each, where the film has one -- so that bar is twice the worst value measured, 1.33e-6.
ABS_BAR = 1.33e-6
REL_BAR = 6.1e-6
# R from the two sides of a stack compares two float32 evaluations, each off the matrix formula by up to the figure above:
# the worst difference measured over the whole grid is 1.61e-6 -- ABS_BAR is missed -- so this bar is twice that.
RECIPROCITY_BAR = 3.22e-6


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def _f32(x):
    return float(np.float32(x))


def matrix64(n, films, thick, n2, lam, cos_in):
    """float64 unpolarised reflectance of the layers (films[i], thick[i]), in the order the wave meets them, between n
    (incidence) and n2: the product of the layers' 2 x 2 characteristic matrices, eta = n cos t for s and n / cos t for p."""
    s = n * math.sqrt(max(0.0, 1.0 - cos_in * cos_in))       # n sin t, invariant
    if s >= n2:
        return 1.0
    cos = lambda m: math.sqrt(1.0 - (s / m) ** 2)
    R = 0.0
    for pol in "sp":
        eta = (lambda m: m * cos(m)) if pol == "s" else (lambda m: m / cos(m))
        M = np.eye(2, dtype=complex)
        for m, d in zip(films, thick):
            delta = 2.0 * math.pi * m * d * cos(m) / lam
            M = M @ np.array([[math.cos(delta), -1j * math.sin(delta) / eta(m)],
                              [-1j * eta(m) * math.sin(delta), math.cos(delta)]])
        B, Cc = M @ np.array([1.0, eta(n2)])
        r = (eta(n) * B - Cc) / (eta(n) * B + Cc)
        R += 0.5 * abs(r) ** 2
    return R


def test_the_matrix_formula_reproduces_the_single_film():
    for n, n2 in ((1.0, 1.67), (1.67, 1.0), (1.0, 1.9)):
        crit = math.sqrt(1.0 - (n2 / n) ** 2) if n > n2 else 0.0
        for m in FILMS:
            for lam in LAMBDAS:
                for d in (0.0, 37.0, lam / (4 * m), 333.0):
                    for c in np.linspace(1.0, crit + 0.02, 9):
                        assert abs(matrix64(n, [m], [d], n2, lam, c) - airy64(n, m, n2, d, lam, c)) <= 1e-12


def _grid():
    """(n, films, thick, n2, lam, cos_in): 2 .. 6 layers, asymmetric stacks, both directions between air and glass 1.45 ..
    1.9, the three lines, incidence to 0.9 of the critical angle (of grazing incidence from the air side)"""
    rng = np.random.default_rng(20261019)
    for N in range(2, 7):
        for _ in range(8):
            films = [float(v) for v in rng.choice(FILMS, N)]
            while len(set(films)) < 2 or films == films[::-1]:
                films = [float(v) for v in rng.choice(FILMS, N)]
            thick = [float(v) for v in rng.uniform(10.0, 400.0, N)]
            for glass in (1.45, 1.67, 1.9):
                for n, n2 in ((1.0, glass), (glass, 1.0)):
                    t_max = 0.9 * (math.asin(n2 / n) if n > n2 else 0.5 * math.pi)
                    for lam in LAMBDAS:
                        for t in np.linspace(0.0, t_max, 10):
                            yield (_f32(n), [_f32(v) for v in films], [_f32(v) for v in thick], _f32(n2), _f32(lam),
                                   _f32(math.cos(t)))


@pytest.fixture(scope="module")
def grid():
    """the grid with the library's and the matrix formula's reflectance, computed once"""
    pkg = _pkg()
    out = []
    for n, films, thick, n2, lam, c in _grid():
        out.append((n, films, thick, n2, lam, c, pkg.coating_stack_reflectance(n, films, thick, n2, lam, c),
                    matrix64(n, films, thick, n2, lam, c)))
    return out


def test_against_the_float64_matrix_formula_on_a_dense_grid(grid):
    """Measured over the 7200 points: max |dR| = 6.62e-7 -- the single film's bar of 5.3e-7 is missed, the bar is twice the
    measured worst, 1.33e-6 -- and a relative error of 1 - R of 1.27e-6 (the single film's bar, 6.1e-6, holds)."""
    worst = [0.0, 0.0]
    for n, films, thick, n2, lam, c, got, want in grid:
        worst[0] = max(worst[0], abs(got[2] - want))
        worst[1] = max(worst[1], abs((1.0 - got[2]) - (1.0 - want)) / (1.0 - want))
    print("max |dR|, max relative error of 1 - R:", worst, "over", len(grid), "points")
    for n, films, thick, n2, lam, c, got, want in grid:
        assert abs(got[2] - want) <= ABS_BAR, (n, films, thick, n2, lam, c, got, want)
        assert abs(got[2] - want) <= REL_BAR * (1.0 - want), (n, films, thick, n2, lam, c, got, want)
        assert got[2] == pytest.approx(0.5 * (got[0] + got[1]), abs=2e-7)


def test_lossless_and_reciprocal(grid):
    """R in [0, 1]; the stack seen from its other side (the layers reversed) at the corresponding angle reflects the same.
    Measured over the 7200 points: the two float32 results differ by at most 1.61e-6 (beyond what the float64 formula itself
    moves for the rounded angle) -- the bar of the grid test, 1.33e-6, is missed, so the bar here is twice the measured
    worst, 3.22e-6."""
    pkg = _pkg()
    worst = 0.0
    for n, films, thick, n2, lam, c, got, want in grid:
        assert all(0.0 <= v <= 1.0 for v in got)
        s = n * math.sqrt(max(0.0, 1.0 - c * c))
        c2 = _f32(math.sqrt(1.0 - (s / n2) ** 2))
        back = pkg.coating_stack_reflectance(n2, films[::-1], thick[::-1], n, lam, c2)
        # (c2 is rounded to float: the reversed call sits at a slightly different angle, judged by the matrix formula)
        slack = abs(matrix64(n2, films[::-1], thick[::-1], n, lam, c2) - want)
        worst = max(worst, abs(back[2] - got[2]) - slack)
        assert abs(back[2] - got[2]) <= RECIPROCITY_BAR + slack, (n, films, thick, n2, lam, c)
    print("max difference between the two sides:", worst)


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("ns", [1.5, 1.67, 1.9])
def test_v_coat_has_no_reflectance_at_its_design_wavelength(lam, ns):
    """two quarter-wave layers with m2 = m1 sqrt(ns): R = ((m2^2 - m1^2 ns) / (m2^2 + m1^2 ns))^2 = 0"""
    pkg = _pkg()
    m1 = 1.38
    m2 = m1 * math.sqrt(ns)
    R = pkg.coating_stack_reflectance(1.0, [m1, m2], [lam / (4 * m1), lam / (4 * m2)], ns, lam, 1.0)
    assert R[2] < 1e-6 and R[0] < 1e-6 and R[1] < 1e-6
    back = pkg.coating_stack_reflectance(ns, [m2, m1], [lam / (4 * m2), lam / (4 * m1)], 1.0, lam, 1.0)
    assert back[2] < 1e-6
    other = [l for l in LAMBDAS if l != lam][0]
    assert pkg.coating_stack_reflectance(1.0, [m1, m2], [lam / (4 * m1), lam / (4 * m2)], ns, other, 1.0)[2] > 1e-4


@pytest.mark.parametrize("where", [0, 1, 2])
def test_a_half_wave_layer_is_absent_at_its_design_wavelength(where):
    pkg = _pkg()
    lam, n2 = 587.6, 1.67
    films, thick = [1.38, 1.63], [70.0, 121.0]
    want = pkg.coating_stack_reflectance(1.0, films, thick, n2, lam, 1.0)[2]
    f3, t3 = list(films), list(thick)
    f3.insert(where, 2.05)
    t3.insert(where, lam / (2 * 2.05))
    got = pkg.coating_stack_reflectance(1.0, f3, t3, n2, lam, 1.0)[2]
    assert abs(got - want) <= ABS_BAR
    assert abs(got - matrix64(1.0, films, thick, n2, lam, 1.0)) <= ABS_BAR


def test_one_layer_is_the_single_film_bit_for_bit():
    pkg = _pkg()
    for n, n2 in ((1.0, 1.67), (1.67, 1.0)):
        for m in (1.38, 2.3):
            for d in (0.0, 99.638, 777.0):
                for c in (1.0, 0.93, 0.8):
                    assert pkg.coating_stack_reflectance(n, [m], [d], n2, 550.0, c) == pkg.coating_reflectance(n, m, n2, d, 550.0, c)
    assert pkg.coating_stack_reflectance(1.0, [], [], 1.67, 550.0, 0.9) == pkg.coating_reflectance(1.0, 1.0, 1.67, 0.0, 550.0, 0.9)
    assert pkg.coating_stack_reflectance(1.67, [1.38, 2.05], [100.0, 50.0], 1.0, 550.0, 0.3) == (1.0, 1.0, 1.0)   # total reflection


def test_two_adjacent_layers_of_one_index_are_the_film_of_the_summed_thickness():
    pkg = _pkg()
    for n, n2 in ((1.0, 1.67), (1.67, 1.0)):
        for m in (1.38, 2.05):
            for lam in LAMBDAS:
                for c in (1.0, 0.95, 0.85):
                    two = pkg.coating_stack_reflectance(n, [m, m], [40.0, 59.638], n2, lam, c)[2]
                    one = pkg.coating_reflectance(n, m, n2, 99.638, lam, c)[2]
                    assert abs(two - one) <= ABS_BAR


def test_a_layer_of_thickness_zero_changes_nothing_bit_for_bit():
    pkg = _pkg()
    films, thick = [1.38, 2.05, 1.63], [99.6, 134.1, 84.4]
    for n, n2 in ((1.0, 1.67), (1.67, 1.0)):
        for c in (1.0, 0.9, 0.8):
            want = pkg.coating_stack_reflectance(n, films, thick, n2, 550.0, c)
            for where in range(4):
                f, t = list(films), list(thick)
                f.insert(where, 1.46)
                t.insert(where, 0.0)
                assert pkg.coating_stack_reflectance(n, f, t, n2, 550.0, c) == want


@pytest.mark.parametrize("args", [
    (1.0, [1.38] * 7, [50.0] * 7, 1.67, 550.0, 1.0),               # more than LF_MAX_COAT_LAYERS layers
    (1.0, [1.38, float("nan")], [50.0, 50.0], 1.67, 550.0, 1.0),
    (1.0, [1.38, 2.05], [50.0, -1.0], 1.67, 550.0, 1.0),
    (1.0, [1.38, 2.05], [50.0, 10001.0], 1.67, 550.0, 1.0),
    (1.2, [1.38, 1.1], [50.0, 50.0], 1.67, 550.0, 1.0),            # a layer below both media
    (1.0, [1.38, 2.05], [50.0, 50.0], 1.67, 0.0, 1.0),
    (1.0, [1.38, 2.05], [50.0, 50.0], 1.67, 550.0, 1.5),
])
def test_refusals(args):
    pkg = _pkg()
    with pytest.raises(pkg.LensFlareError):
        pkg.coating_stack_reflectance(*args)


# ---- the lens-file syntax (the Python parser)
def _src():
    return open(os.path.join(ROOT, "lens-flare_amd", "data", "dgauss11.lens")).read()


def test_layer_lines_accumulate_in_order_and_one_index_is_broadcast(tmp_path):
    pkg = _pkg()
    p = tmp_path / "x.lens"
    p.write_text("lambda_nm 656.3 587.6 486.1\n" + _src() +
                 "layer 0 99.6 1.38\nlayer 2 50 1.46\nlayer 0 134.1 2.04 2.05 2.07\nlayer 0 84.4 1.63\ncoating 4 99.638 1.38\n")
    lens = pkg.load_lens_file(str(p))
    assert "coatings" not in lens
    c = lens["coating_stacks"]
    assert np.allclose(c["lambda_nm"], LAMBDAS)
    assert list(c["n_layers"]) == [3, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0]
    assert c["thickness_nm"].shape == (pkg.MAX_COAT_LAYERS, 11) and c["index"].shape == (pkg.MAX_COAT_LAYERS, 3, 11)
    assert np.allclose(c["thickness_nm"][:3, 0], [99.6, 134.1, 84.4]) and np.all(c["thickness_nm"][3:, 0] == 0)
    assert np.all(c["index"][0, :, 0] == np.float32(1.38)) and np.all(c["index"][2, :, 0] == np.float32(1.63))
    assert np.allclose(c["index"][1, :, 0], [2.04, 2.05, 2.07])
    assert c["thickness_nm"][0, 2] == np.float32(50) and c["thickness_nm"][0, 4] == np.float32(99.638)   # the coating line: one layer
    bare = pkg.load_lens_file("dgauss11.lens")
    for k in ("radius", "thickness", "ior", "semi_aperture"):
        assert np.array_equal(lens[k], bare[k])


def test_layer_lines_need_lambda_nm(tmp_path):
    pkg = _pkg()
    p = tmp_path / "x.lens"
    p.write_text(_src() + "layer 0 100 1.38\n")
    with pytest.raises(ValueError, match="lambda_nm"):
        pkg.load_lens_file(str(p))


def test_seven_layers_are_refused(tmp_path):
    pkg = _pkg()
    p = tmp_path / "x.lens"
    p.write_text("lambda_nm 656.3 587.6 486.1\n" + _src() + "layer 0 50 1.38\n" * 6)
    assert pkg.load_lens_file(str(p))["coating_stacks"]["n_layers"][0] == 6
    p.write_text("lambda_nm 656.3 587.6 486.1\n" + _src() + "layer 0 50 1.38\n" * 7)
    with pytest.raises(ValueError, match="layers"):
        pkg.load_lens_file(str(p))


@pytest.mark.parametrize("order", ["layer_first", "coating_first", "coating_of_thickness_zero"])
def test_layer_and_coating_on_one_interface_are_refused(tmp_path, order):
    pkg = _pkg()
    p = tmp_path / "x.lens"
    lines = ["layer 2 50 1.46\n", "coating 2 0 1.38\n" if order == "coating_of_thickness_zero" else "coating 2 99.638 1.38\n"]
    p.write_text("lambda_nm 656.3 587.6 486.1\n" + _src() + "".join(lines if order == "layer_first" else lines[::-1]))
    with pytest.raises(ValueError, match="coating"):
        pkg.load_lens_file(str(p))


def test_multicoated_lens_file():
    """dgauss11_multicoated.lens: dgauss11.lens with a stack on the eight air-glass interfaces, the low index facing
    the air; the reflectances its header states are the matrix formula's"""
    pkg = _pkg()
    path = os.path.join(ROOT, "lens-flare_amd", "data", "dgauss11_multicoated.lens")
    lens = pkg.load_lens_file("dgauss11_multicoated.lens")
    bare = pkg.load_lens_file("dgauss11.lens")
    for k in ("radius", "thickness", "ior", "semi_aperture"):
        assert np.array_equal(lens[k], bare[k])
    c = lens["coating_stacks"]
    coated = [0, 1, 2, 4, 6, 8, 9, 10]
    assert np.allclose(c["lambda_nm"], LAMBDAS)
    assert all(c["n_layers"][k] >= 2 for k in coated) and all(c["n_layers"][k] == 0 for k in (3, 5, 7))
    ior = lens["ior"]
    stated = {}
    for line in open(path):
        m = re.match(r"#\s+interface\s+(\d+)\s*:\s*R\s*=\s*([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)\s*%", line)
        if m:
            stated[int(m.group(1))] = [float(m.group(i)) for i in (2, 3, 4)]
    assert sorted(stated) == coated
    for k in coated:
        N = c["n_layers"][k]
        before = np.ones(3) if k == 0 else ior[:, k - 1].astype(np.float64)     # the medium on the scene side
        after = ior[:, k].astype(np.float64)
        air_in_front = before[1] == 1.0
        films = c["index"][:N, :, k].astype(np.float64)
        # the low index faces the air
        assert (films[0, 1] < films[-1, 1]) == air_in_front
        for l in range(3):
            R = matrix64(before[l], list(films[:, l]), list(c["thickness_nm"][:N, k].astype(np.float64)), after[l], LAMBDAS[l], 1.0)
            assert 100.0 * R == pytest.approx(stated[k][l], abs=6e-4), (k, l)
            bare_R = ((before[l] - after[l]) / (before[l] + after[l])) ** 2
            assert R < 0.15 * bare_R
