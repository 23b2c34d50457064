"""The float64 tracer (oracle/lf_geo_f64.c) under films and the bilinear stop (lfo.g64_set_films,
lfo.g64_set_mask_filter), CPU only: what makes it a reference for the coated and filtered lens camera
(tests/test_gpu_lens_camera_variants.py).  Its film is Airy's formula in complex arithmetic and its bilinear
stop is written from DESIGN.md section 4's contract; neither shares an expression with the device.  Here they
meet (1) the float64 Airy formula of tests/test_coatings_cpu.py, written a third time and differently,
(2) their closed forms, (3) the HOST evaluations of the device's float32 arithmetic (lf_coating_reflectance,
lf_mask_lookup) within the bounds DESIGN.md states for those, and (4) the slope allowance's own promise."""
import math

import numpy as np
import pytest

from oracle import lfo
from test_coatings_cpu import GLASS, LAMBDAS, airy64, bare64
from test_mask_filter_cpu import _u_of, bilinear64

NG = float(np.float32(GLASS))
M_FILM = float(np.float32(1.38))


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def _slab():
    """one flat interface at z = 0, air in front (z < 0), glass behind"""
    return dict(n=1, stop=-1, radius=np.array([0.0], np.float32), thickness=np.array([10.0], np.float32),
                ior=np.array([[GLASS]] * 3, np.float32), semi_aperture=np.array([1e3], np.float32), sensor_width_mm=36.0)


def _plate(t=5.0):
    """two flat interfaces: air | glass (t mm) | air, the sensor 10 mm behind"""
    return dict(n=2, stop=-1, radius=np.zeros(2, np.float32), thickness=np.array([t, 10.0], np.float32),
                ior=np.array([[GLASS, 1.0]] * 3, np.float32), semi_aperture=np.array([1e3, 1e3], np.float32),
                sensor_width_mm=36.0)


def _films(thickness, index, n=1):
    return dict(lambda_nm=np.array(LAMBDAS, np.float32), thickness_nm=np.full(n, thickness, np.float32),
                index=np.full((3, n), index, np.float32))


def _event(L, lam, cos_in, into_glass, mirror):
    """weight after one event of a ray that meets the slab's interface at cos_in, from the air or from the glass"""
    s = math.sqrt(max(0.0, 1.0 - cos_in * cos_in))
    p, d = ([0.0, 0.0, -1.0], [s, 0.0, cos_in]) if into_glass else ([0.0, 0.0, 1.0], [s, 0.0, -cos_in])
    st, _, _, w = lfo.g64_glass_event(L, lam, 0, int(mirror), p, d)
    return st, w


@pytest.fixture()
def films():
    """install films for one test; the default (none) is restored whatever happens"""
    try:
        yield lfo.g64_set_films
    finally:
        lfo.g64_set_films(None)


@pytest.fixture()
def bilinear():
    lfo.g64_set_mask_filter(1)
    try:
        yield
    finally:
        lfo.g64_set_mask_filter(0)


# ---- the film ---------------------------------------------------------------------------------------------------

def test_slab_against_airy64(films):
    """normal incidence at quarter- and half-wave, an angle sweep to 0.9 of the critical angle, both directions of
    travel, mirror and refraction: two float64 evaluations of one formula, 1e-12 relative"""
    L = lfo.g64_lens(_slab())
    worst = 0.0
    for into_glass in (True, False):
        n1, n2 = (1.0, NG) if into_glass else (NG, 1.0)
        t_max = 0.9 * (math.asin(n2 / n1) if n1 > n2 else math.pi / 2)
        for lam, lam_nm in enumerate(LAMBDAS):
            lam_nm = float(np.float32(lam_nm))
            for d in (lam_nm / (4 * M_FILM), lam_nm / (2 * M_FILM), 99.6, 333.0):
                d = float(np.float32(d))
                films(_films(d, 1.38))
                for c in [1.0] + [math.cos(t) for t in np.linspace(0.0, t_max, 25)]:
                    want = airy64(n1, M_FILM, n2, d, lam_nm, c)
                    st, R = _event(L, lam, c, into_glass, True)
                    assert st == 0 and R == pytest.approx(want, rel=1e-12), (into_glass, lam, d, c)
                    st, T = _event(L, lam, c, into_glass, False)
                    assert st == 0 and T == pytest.approx(1.0 - want, rel=1e-12)
                    worst = max(worst, abs(R / want - 1.0))
            # the closed forms at normal incidence: a quarter-wave film, an absent half-wave film
            films(_films(np.float32(lam_nm / (4 * M_FILM)), 1.38))
            assert _event(L, lam, 1.0, into_glass, True)[1] == pytest.approx(
                ((n1 * n2 - M_FILM ** 2) / (n1 * n2 + M_FILM ** 2)) ** 2, rel=1e-6)     # (d is a float32: not exactly lambda / 4m)
            films(_films(np.float32(lam_nm / (2 * M_FILM)), 1.38))
            assert _event(L, lam, 1.0, into_glass, True)[1] == pytest.approx(((n1 - n2) / (n1 + n2)) ** 2, rel=1e-6)
    print("film against airy64: worst relative deviation", worst)


def test_plate_paths_against_airy64(films):
    """whole paths (lfo.g64_trace_ray) through a plate with a film on each face: the primary path's transmission and
    the ghost of the two faces, each face met from its own side at its own angle"""
    lens = _plate()
    zs = lfo.g64_sensor_z(lens)
    d_nm = float(np.float32(99.6))
    films(_films(d_nm, 1.38, n=2))
    for lam, lam_nm in enumerate(LAMBDAS):
        lam_nm = float(np.float32(lam_nm))
        for theta in (0.0, 0.2, 0.6, 1.0):
            ca = math.cos(theta)                                   # in air
            cg = math.sqrt(1.0 - (math.sin(theta) / NG) ** 2)      # in the glass
            R_in = airy64(1.0, M_FILM, NG, d_nm, lam_nm, ca)       # air -> glass
            R_out = airy64(NG, M_FILM, 1.0, d_nm, lam_nm, cg)      # glass -> air
            d = [math.sin(theta), 0.0, -ca]
            st, _, de, w, ne = lfo.g64_trace_ray(lens, lam, -1, -1, [0.0, 0.0, zs], d)
            assert st == 0 and ne == 2 and w == pytest.approx((1.0 - R_in) * (1.0 - R_out), rel=1e-12)
            assert de[0] == pytest.approx(d[0], abs=1e-12)        # (films never bend a ray)
            # ghost (0, 1): in through face 1, mirror on face 0 (from the glass), mirror on face 1 (from the glass), out
            st, _, _, w, ne = lfo.g64_trace_ray(lens, lam, 0, 1, [0.0, 0.0, zs], d)
            assert st == 0 and ne == 4
            assert w == pytest.approx((1.0 - R_in) * R_out * R_out * (1.0 - R_out), rel=1e-12)
    # reciprocity is why R_in and R_out above agree at matching angles; total reflection stays 1 and kills a refraction
    L = lfo.g64_lens(_slab())
    films(_films(d_nm, 1.38))
    assert _event(L, 1, 0.3, False, True) == (0, 1.0)
    assert _event(L, 1, 0.3, False, False)[0] == 3


def test_two_bare_equivalents(films):
    """a film of the incidence medium's index is the bare interface, and so is a film of no thickness"""
    L = lfo.g64_lens(_slab())
    for into_glass in (True, False):
        n1, n2 = (1.0, NG) if into_glass else (NG, 1.0)
        crit = math.sqrt(1.0 - (n2 / n1) ** 2) if n1 > n2 else 0.0
        for c in np.linspace(1.0, crit + 0.05, 12):
            films(None)
            bare = _event(L, 1, c, into_glass, True)[1]
            assert bare == pytest.approx(bare64(n1, n2, c), rel=1e-12)
            films(_films(321.0, n1))
            assert _event(L, 1, c, into_glass, True)[1] == pytest.approx(bare, rel=1e-12)
            films(_films(0.0, 1.38))
            assert _event(L, 1, c, into_glass, True)[1] == bare
            films(_films(0.0, 1.38))
            assert _event(L, 1, c, into_glass, False)[1] == 1.0 - bare


def test_wrapper_rounds_through_float32_and_clears(films):
    L = lfo.g64_lens(_slab())
    bare = _event(L, 0, 0.9, True, True)[1]
    films(dict(lambda_nm=LAMBDAS, thickness_nm=[99.6], index=1.38))          # one index for all, Python floats
    got = _event(L, 0, 0.9, True, True)[1]
    assert got == airy64(1.0, M_FILM, NG, float(np.float32(99.6)), float(np.float32(LAMBDAS[0])), 0.9) or \
        got == pytest.approx(airy64(1.0, M_FILM, NG, float(np.float32(99.6)), float(np.float32(LAMBDAS[0])), 0.9), rel=1e-13)
    assert got != pytest.approx(airy64(1.0, 1.38, GLASS, 99.6, LAMBDAS[0], 0.9), rel=1e-11)   # not the unrounded numbers
    films(None)
    assert _event(L, 0, 0.9, True, True)[1] == bare


def test_film_against_the_hosts_float32_arithmetic(films):
    """the grid of test_coatings_cpu.py::test_against_float64_airy_on_a_dense_grid, the tracer in airy64's place, within
    what DESIGN.md section 4 ("Coatings") states for that comparison: |dR| <= 5.3e-7 away from the critical angle,
    <= 3.9e-6 near it, <= 6.1e-6 relative where R >= 1e-3.  Measured here: 5.3e-7, 3.9e-6, 6.1e-6 (printed)."""
    pkg = _pkg()
    L = lfo.g64_lens(_slab())
    f32 = lambda x: float(np.float32(x))   # noqa: E731
    worst = [0.0, 0.0, 0.0]
    for into_glass in (True, False):
        n, n2 = (1.0, NG) if into_glass else (NG, 1.0)
        crit = math.sqrt(1.0 - (n2 / n) ** 2) if n > n2 else 0.0
        for m in (1.38, 2.3):
            for lam, lam_nm in enumerate(LAMBDAS):
                for d in np.linspace(0.0, 1.25 * lam_nm, 21):
                    films(_films(d, m))
                    for c in np.concatenate([np.linspace(1.0, crit + 0.05, 40), np.linspace(crit + 0.05, crit + 1e-3, 12)]):
                        a = [f32(v) for v in (n, m, n2, d, lam_nm, c)]
                        got = pkg.coating_reflectance(*a)[2]
                        st, want = _event(L, lam, a[5], into_glass, True)
                        assert st == 0
                        err = abs(got - want)
                        k = 1 if a[5] < crit + 0.05 else 0
                        worst[k] = max(worst[k], err)
                        if want >= 1e-3:
                            worst[2] = max(worst[2], err / want)
    print("host float32 against the tracer's film: max |dR| far / near the critical angle, max relative:", worst)
    assert worst[0] <= 5.3e-7 * 1.01 and worst[1] <= 3.9e-6 * 1.01 and worst[2] <= 6.1e-6 * 1.01, worst


# ---- the filtered stop ------------------------------------------------------------------------------------------

def _stop_only(h=1.0):
    return dict(n=1, stop=0, radius=np.array([0.0], np.float32), thickness=np.array([10.0], np.float32),
                ior=np.array([[1.0]] * 3, np.float32), semi_aperture=np.array([h], np.float32), sensor_width_mm=36.0)


def _at(t, u, v, h=1.0, **eps):
    """the tracer's (dead, weight, fragile, allowance) of a ray that meets the stop's plane at (u, v) h, straight on"""
    st, _, _, w, _, frag, _, slope = lfo.g64_trace_ray_slope(_stop_only(h), 1, -1, -1, [float(np.float32(u)) * h,
                                                             float(np.float32(v)) * h, 10.0], [0.0, 0.0, -1.0], 1.0, t, **eps)
    return st, w, frag, slope


def _points():
    """the points of tests/test_mask_filter_cpu.py: (texels, u, v) -- centres, borders and clamps, negative texels, the
    liveness rule, random points"""
    out = []
    t = np.random.default_rng(1).random((4, 8)).astype(np.float32)
    out += [(t, _u_of(i + 0.5, 8), _u_of(j + 0.5, 4)) for j in range(4) for i in range(8)]
    t = np.random.default_rng(2).random((4, 8)).astype(np.float32) + 0.1
    out += [(t, u, _u_of(1.5, 4)) for u in (-1.0, _u_of(0.25, 8), -1.5, 1.0, _u_of(7.75, 8), 2.0)]
    out += [(t, u, 0.0) for u in (-1.0, _u_of(0.25, 8), _u_of(0.4, 8), 1.0, _u_of(7.75, 8))]
    out += [(t, _u_of(2.5, 8), v) for v in (-1.0, -3.0, 1.0, _u_of(3.6, 4), _u_of(0.2, 4), 7.0)]
    out += [(np.array([[0.625]], np.float32), u, v) for u, v in ((0.0, 0.0), (-0.9, 0.3), (5.0, -5.0))]
    t = np.array([[-1.0, 0.5, -2.0, -3.0]], np.float32)
    out += [(t, _u_of(f, 4), 0.0) for f in (1.0, 3.0, 3.5, 0.2, 2.2)]
    t = np.array([[0.0, 0.0, 1.0, 1.0]], np.float32)
    out += [(t, _u_of(f, 4), 0.0) for f in (1.5, 1.75, 1.4375, 2.0, 0.5)]       # fx = 0 beside an open texel; all closed
    out += [(t.T.copy(), 0.0, _u_of(f, 4)) for f in (1.5, 1.25, 1.75)]
    out += [(np.zeros((4, 4), np.float32), 0.1, -0.2), (-np.ones((3, 5), np.float32), 0.3, 0.3)]   # the all-closed footprint
    rng = np.random.default_rng(5)
    t = rng.random((5, 7)).astype(np.float32)
    out += [(t, u, v) for u, v in rng.uniform(-1.0, 1.0, (1000, 2)).astype(np.float32)]
    return out


def test_filtered_stop_against_mask_lookup(bilinear):
    """value within 2 (3 + 2 w) 2^-24 of lf_mask_lookup, liveness exactly; outside the housing the ray is dead whatever
    the mask says (the housing test is unchanged)"""
    pkg = _pkg()
    n_in = n_out = n_dead = 0
    worst = 0.0
    for t, u, v in _points():
        u, v = float(np.float32(u)), float(np.float32(v))
        st, w, frag, slope = _at(t, u, v)
        rho = math.hypot(u, v)
        if rho > 1.0:
            assert st == 1 and w == 0.0
            n_out += 1
            continue
        if abs(rho - 1.0) < 1e-3:
            continue                                   # (on the rim: the housing's own fragile decision)
        value, alive = pkg.mask_lookup(t, u, v, pkg.MASK_BILINEAR)
        assert (st == 0) == bool(alive) and st in (0, 1), (u, v, st, alive)
        want64, alive64 = bilinear64(t, u, v)
        assert bool(alive) == bool(alive64)
        if alive:
            bound = 2.0 * (3 + 2 * t.shape[1]) * 2.0 ** -24
            worst = max(worst, abs(w - value))
            assert abs(w - value) <= bound, (u, v, w, value)
            assert w == pytest.approx(want64, abs=1e-14)
            n_in += 1
        else:
            assert w == 0.0
            n_dead += 1
    print(f"filtered stop: {n_in} alive points, worst |tracer - lf_mask_lookup| {worst:.2e}; {n_dead} closed, {n_out} outside the housing")
    assert n_in > 800 and n_dead >= 6 and n_out >= 4
    # the two named cases, spelled out: fx = 0 beside an open texel is alive with weight 0; the all-closed footprint is dead
    t = np.array([[0.0, 0.0, 1.0, 1.0]], np.float32)
    assert _at(t, _u_of(1.5, 4), 0.0)[:2] == (0, 0.0)
    assert _at(t, _u_of(1.4375, 4), 0.0)[:2] == (1, 0.0)


def test_nearest_is_untouched_and_the_filter_is_a_setting():
    t = np.array([[0.0, 0.0, 1.0, 1.0]], np.float32)
    assert _at(t, _u_of(1.75, 4), 0.0)[:2] == (1, 0.0)               # nearest: texel 1, closed
    lfo.g64_set_mask_filter(1)
    try:
        assert _at(t, _u_of(1.75, 4), 0.0)[:2] == (0, 0.25)
    finally:
        lfo.g64_set_mask_filter(0)
    st, w, frag, slope = _at(t, _u_of(1.75, 4), 0.0)
    assert (st, w, slope) == (1, 0.0, 0.0)


def test_no_texel_edge_is_fragile_under_the_filter(bilinear):
    """nearest calls a ray within eps_texel of an edge between unlike texels fragile (cause bit 2); the bilinear weight is
    continuous there, so the ray is not fragile and carries a slope allowance instead"""
    E = np.zeros((8, 8), np.float32)
    E[:, 4:] = 1.0
    u = _u_of(4.0 + 1e-3, 8)                      # on the edge between texels 3 and 4: the middle of the bilinear ramp
    st, w, frag, slope = _at(E, u, 0.01)
    assert st == 0 and frag == 0 and w == pytest.approx(0.501, abs=1e-6) and slope > 0.0
    lfo.g64_set_mask_filter(0)
    assert _at(E, u, 0.01)[2] == 1


def test_slope_allowance_covers_the_move(bilinear):
    """A hard edge, and a point in the edge's half texel.  delta = eps_mm in texels (eps_mm / stop_h x 0.5 mw): two rays
    delta / 2 to either side of the point differ in weight by no more than the allowance the tracer reports for either.
    Also across the border of a cell -- where the bilinear's slope jumps and where the open texel enters the footprint
    (one ray dead, the other alive) -- and across the edge of a texel, where nearest would call both fragile."""
    E = np.zeros((8, 8), np.float32)
    E[:, 4:] = 1.0
    eps_mm, h = 5e-4, 2.0
    delta = eps_mm / h * 0.5 * 8
    M = np.random.default_rng(3).uniform(0.25, 1.0, (8, 8)).astype(np.float32)
    n = 0
    for mask in (E, E.T.copy(), M):
        for f in (3.75, 3.6, 3.5, 3.5 + 0.3 * delta, 4.0, 4.5, 4.5 - 0.2 * delta, 3.9):
            for g in (4.2, 4.5, 2.5 + 0.1 * delta):
                for axis in (0, 1):
                    pts = []
                    for side in (-0.5, 0.5):
                        fu, fv = (f + side * delta, g) if axis == 0 else (g, f + side * delta)
                        p = [(2.0 * fu / 8 - 1.0) * h, (2.0 * fv / 8 - 1.0) * h, 10.0]
                        st, _, _, w, _, frag, _, slope = lfo.g64_trace_ray_slope(_stop_only(h), 1, -1, -1, p, [0.0, 0.0, -1.0],
                                                                                 1.0, mask, eps_mm=eps_mm)
                        pts.append((w if st == 0 else 0.0, slope, st, frag))
                    (wa, sa, sta, fa), (wb, sb, stb, fb) = pts
                    assert abs(wa - wb) <= min(sa, sb) * (1.0 + 1e-9) + 1e-15, (f, g, axis, pts)
                    if sta != stb:
                        assert fa == 1 and fb == 1      # the liveness decision itself is flagged on both sides
                    n += wa != wb
    assert n > 80                                   # (the pairs that move along a hard edge see no change)
    # the allowance is first order in delta, not a blanket: a tenth of the tolerance gives a tenth of it
    a = lfo.g64_trace_ray_slope(_stop_only(h), 1, -1, -1, [-0.125 * h, 0.01, 10.0], [0.0, 0.0, -1.0], 1.0, E, eps_mm=eps_mm)[7]
    b = lfo.g64_trace_ray_slope(_stop_only(h), 1, -1, -1, [-0.125 * h, 0.01, 10.0], [0.0, 0.0, -1.0], 1.0, E, eps_mm=eps_mm / 10)[7]
    assert a == pytest.approx(delta, rel=1e-12) and b == pytest.approx(delta / 10, rel=1e-12)


def test_allowance_follows_the_ray_through_the_lens(bilinear, films):
    """the double Gauss: frag / the potential-weight column carry the allowance times what the interfaces after the stop
    transmit, and nothing else changes -- geometry, fate and weight are those of a ray traced without it"""
    pkg = _pkg()
    lens = pkg.load_lens_file("dgauss11_coated.lens")
    M = np.random.default_rng(12).uniform(0.25, 1.0, (16, 16)).astype(np.float32)
    g = (np.arange(12) + 0.5) / 6.0 - 1.0
    uv = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2).astype(np.float32)
    xy = np.tile(np.float32([3.0, -2.0]), (len(uv), 1))
    films(lens["coatings"])
    a = lfo.g64_lens_rays(lens, 1, xy, uv, M)
    tight = lfo.g64_lens_rays(lens, 1, xy, uv, M, eps_mm=5e-5)
    alive = (a[:, 9] == 0) & (a[:, 8] == 0) & (tight[:, 8] == 0)
    assert alive.sum() > 30
    assert np.array_equal(a[alive, :7], tight[alive, :7])
    sa, st = a[alive, 7] - a[alive, 6], tight[alive, 7] - tight[alive, 6]
    inner = sa < 0.02 * a[alive, 6]                                  # (away from a cell's border both see one cell's slope)
    assert inner.sum() > 20 and np.allclose(sa[inner], 10.0 * st[inner], rtol=1e-9)
    assert (sa > 0).all() and (sa < 0.05 * a[alive, 6]).all()
    # films change weights only
    films(None)
    b = lfo.g64_lens_rays(lens, 1, xy, uv, M)
    assert np.array_equal(a[alive, :6], b[alive, :6]) and np.array_equal(a[:, 9], b[:, 9])
    ratio = a[alive, 6] / b[alive, 6]
    assert (ratio > 1.3).all() and (ratio < 1.8).all()    # eight faces reflect ~1.5 % instead of 6-8 %: x 1.62
