"""What tests/test_gpu_lens_camera_surfaces.py and tests/test_lens_camera_surfaces_cpu.py share: the frame's shape and pose, the
recorded lenses, the float64 tracers' primary path at given starts (cached: one trace of 24 576 rays takes seconds), the
fragile-sample rule and the composition of a tracer frame with its allowance.  Not a test module."""
import numpy as np

import asphere_ref as ar
import biconic_ref as br
from test_aspheres_cpu import COS_MIN, _surfaces, _yardstick
from test_biconics_cpu import _D, _cases
from test_gpu_lens_camera import LIGHTS, SPHERES, TRIS, compose, look_at

W, H, NS, WPM = 48, 32, 16, 0.004          # tests/test_gpu_lens_camera_variants.py: strata, sub-cells, several wave tiles
POS = [0.3, 0.2, 1.0]
C2W = look_at(POS, [0.0, -0.2, -5.5])
ODD = (37, 21, 7)                          # no multiple of the wave tile; 7 samples: 4 stratified, 3 not
ALLOWANCE_CAP = 0.02                       # of the frame's summed value
ONES = np.ones((8, 8), np.float32)         # the float64 Python tracers know no fragility at texel edges


def package():
    import __graft_entry__ as g
    return g.load_package()


_cache = {}


def lens_of(name):
    """'asph' / 'anam' / 'plain', and '<name>-dropped': the same prescription with its records taken out"""
    if name not in _cache:
        pkg = package()
        base, _, dropped = name.partition("-")
        lens = pkg.load_lens_file({"asph": "dgauss11_asph.lens", "anam": "dgauss11_anamorphic.lens", "plain": "dgauss11.lens"}[base])
        if dropped:
            lens = {k: v for k, v in lens.items() if k not in ("aspheres", "biconics")}
        _cache[name] = lens
    return _cache[name]


def films_of(name):
    """dgauss11_coated.lens's films on the double Gauss's eleven interfaces; on the anamorphic lens (four more in front) also a
    quarter-wave MgF2 film on the two cylinder faces, as tests/test_gpu_biconics.py coats it"""
    c = package().load_lens_file("dgauss11_coated.lens")["coatings"]
    n = int(lens_of(name)["n"])
    if n == len(c["thickness_nm"]):
        return c
    th = np.zeros(n, np.float32); idx = np.zeros((c["index"].shape[0], n), np.float32)
    th[n - 11:] = c["thickness_nm"]; idx[:, n - 11:] = c["index"]
    th[[1, 2]] = 100.0; idx[:, [1, 2]] = 1.38
    return dict(lambda_nm=c["lambda_nm"], thickness_nm=th, index=idx)


def yardstick_D(name):
    """the event yardstick D as tests/test_gpu_aspheres.py and tests/test_gpu_biconics.py take it"""
    if name.startswith("anam"):
        return max(_D(s) for s in _cases()[:2])
    return max(_yardstick(s) for s in _surfaces())


def trace(name, lam, starts, tag, films=True):
    """the primary path of the tracer at starts (n, 4) {X, Y, pa, pb} under a mask of ones, traced ONCE per (lens, wavelength,
    tag) with the lens's films: the weight with them in column 6 of [0], the bare lens's weight in [4]"""
    key = ("trace", name, lam, tag)
    if key not in _cache:
        s = np.asarray(starts, np.float32).reshape(-1, 4)
        _cache[key] = br.trace_path(lens_of(name), lam, -1, -1, s[:, 0:2], s[:, 2:4], ONES, films_of(name) if films else None)
    return _cache[key]


def tracer_samples(t, filmed, shape):
    """(n_pix, ns, 8) samples of a trace as compose takes them, with the filmed or the bare weight in column 6"""
    smp = t[0].copy()
    if not filmed:
        smp[:, 6] = t[4]
    return smp.reshape(shape + (8,))


def fragile(name, t):
    """a sample is fragile where the tracer met an aperture rim within 4 D n_ev or an incidence cosine of 0.05 or less"""
    n_ev = int(lens_of(name)["n"])
    return (t[2] <= 4 * yardstick_D(name) * n_ev) | (t[1] <= COS_MIN)


def tracer_frame(name, t, filmed, shape, z_ref, exposure, pose=(C2W, POS, WPM), scene=(SPHERES, TRIS, LIGHTS)):
    """(frame, allowance), each (n_pix, 3), of one wavelength's trace.  A fragile sample may go either way in float32: one the
    tracer passed can add or remove its weight times the radiance ITS ray finds; one the tracer killed has no weight -- the
    frame's largest weight, times the radiance its ray finds too: the tracer marches a ray on past the rim that stopped it,
    the way float32 would send it had it passed.  A ray that went on nowhere gets no allowance: it missed a later surface by
    more than a quarter of its clear aperture (asphere_ref.r_limit) or was totally reflected there, so float32 loses it too,
    whichever way the rim test that stopped it first falls."""
    n_pix, ns = shape
    lens = lens_of(name)
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


def crude_allowance(name, t, filmed):
    """fragile count x largest weight / summed weight: an upper bound of the allowance's share of a frame of even radiance"""
    w = t[0][:, 6] if filmed else t[4]
    return float(fragile(name, t).sum() * w.max() / w.sum())


def random_starts(seed, w=W, h=H, ns=NS, sensor_w_mm=36.0):
    """(w h, ns, 4): a uniformly random sensor point inside each pixel and a uniformly random point of the pupil square -- the
    device's sample_start_in without its strata, no device needed"""
    rng = np.random.default_rng(seed)
    pitch = np.float32(sensor_w_mm) / np.float32(w)
    y, x = np.divmod(np.arange(w * h), w)
    jx, jy, pa, pb = (rng.random((w * h, ns)) for _ in range(4))
    X = -((x[:, None] + jx) - 0.5 * w) * pitch
    Y = -((y[:, None] + jy) - 0.5 * h) * pitch
    return np.stack([X, Y, 2 * pa - 1, 2 * pb - 1], axis=-1).astype(np.float32)
