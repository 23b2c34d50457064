"""A float64 numpy tracer for biconic interfaces (cylinders, toroids) -- the reference of tests/test_biconics_cpu.py and
tests/test_gpu_biconics.py, written independently of the kernels' event (lens-flare_amd/csrc/lf_biconic.h):

  * the intersection is BRACKETED between the two planes that bound the sag over the clear disc, the span scanned for its
    first change of sign and that interval closed by the ILLINOIS variant of regula falsi (a bracketing secant method) to
    1e-13 mm -- the kernel starts from a quadric's root and only ever runs Newton;
  * the slopes are the quotient rule's two terms, z_x = 2 cx x / (1 + root) + A (1 + kx) cx^2 x / (root (1 + root)^2)
    (the header folds them into one factor); check_gradient() compares them with a central difference of the sag;
  * rays carry UNIT directions and absolute z; Snell's law and the mirror are the unit-direction vector forms.

The spherical and aspheric rows of a lens, the lens geometry, the pupil map and the films are tests/asphere_ref.py's.
Fates as there: 0 alive, 1 missed, 2 outside the clear aperture, 3 totally reflected, 4 blocked by the stop mask."""
import numpy as np

import asphere_ref as ar
from asphere_ref import ALIVE, MISSED, APERTURE, TIR, CLIPPED  # noqa: F401


def sag(cx, cy, kx, ky, x, y):
    """z, dz/dx, dz/dy in float64; NaN beyond the conic's domain."""
    x = np.asarray(x, np.float64); y = np.asarray(y, np.float64)
    A = cx * x * x + cy * y * y
    with np.errstate(invalid="ignore", divide="ignore"):
        root = np.sqrt(1.0 - (1.0 + kx) * cx * cx * x * x - (1.0 + ky) * cy * cy * y * y)
        z = A / (1.0 + root)
        common = A / (root * (1.0 + root) ** 2)
        zx = 2.0 * cx * x / (1.0 + root) + common * (1.0 + kx) * cx * cx * x
        zy = 2.0 * cy * y / (1.0 + root) + common * (1.0 + ky) * cy * cy * y
    return z, zx, zy


def r_limit(cx, cy, kx, ky, h):
    """the radius up to which the bracket follows the true surface: a quarter beyond the clear aperture, inside the domain"""
    lim = 1.25 * h
    q = max((1.0 + kx) * cx * cx, (1.0 + ky) * cy * cy)
    if q > 0:
        lim = min(lim, 0.999 / np.sqrt(q))
    return lim


def check_gradient(cx, cy, kx, ky, h, n=24, eps=1e-6):
    """largest |analytic slope - central difference| over the clear aperture"""
    g = np.linspace(-h, h, n)
    x, y = [a.ravel() for a in np.meshgrid(g, g)]
    keep = x * x + y * y <= h * h
    x, y = x[keep], y[keep]
    _, zx, zy = sag(cx, cy, kx, ky, x, y)
    dx = (sag(cx, cy, kx, ky, x + eps, y)[0] - sag(cx, cy, kx, ky, x - eps, y)[0]) / (2 * eps)
    dy = (sag(cx, cy, kx, ky, x, y + eps)[0] - sag(cx, cy, kx, ky, x, y - eps)[0]) / (2 * eps)
    return float(max(np.max(np.abs(zx - dx)), np.max(np.abs(zy - dy))))


def slope_turn(cx, cy, kx, ky, h, n=129):
    """the largest rate of change of the slope (dz/dx, dz/dy) over the clear aperture, over BOTH meridians: the Frobenius
    norm of the sag's Hessian (it bounds the largest turn per mm in any direction), by central differences of the slopes"""
    g = np.linspace(-h, h, n)
    x, y = [a.ravel() for a in np.meshgrid(g, g)]
    keep = x * x + y * y <= h * h
    x, y = x[keep], y[keep]
    e = 1e-5
    _, axp, ayp = sag(cx, cy, kx, ky, x + e, y); _, axm, aym = sag(cx, cy, kx, ky, x - e, y)
    _, bxp, byp = sag(cx, cy, kx, ky, x, y + e); _, bxm, bym = sag(cx, cy, kx, ky, x, y - e)
    zxx = (axp - axm) / (2 * e); zxy = (ayp - aym) / (2 * e); zyx = (bxp - bxm) / (2 * e); zyy = (byp - bym) / (2 * e)
    return float(np.nanmax(np.sqrt(zxx ** 2 + zxy ** 2 + zyx ** 2 + zyy ** 2)))


def intersect(p, d, zv, cx, cy, kx, ky, h, scan=513):
    """ray parameter t of the first crossing of p + t d with the surface of vertex z zv; NaN where there is none"""
    p = np.asarray(p, np.float64); d = np.asarray(d, np.float64)
    rl = r_limit(cx, cy, kx, ky, h)
    g = np.linspace(-rl, rl, 257)
    gx, gy = np.meshgrid(g, g)
    inside = gx * gx + gy * gy <= rl * rl
    zs = sag(cx, cy, kx, ky, gx[inside], gy[inside])[0]
    zlo, zhi = float(np.min(zs)) - 1e-9, float(np.max(zs)) + 1e-9

    def f(t):
        x = p[:, 0] + t * d[:, 0]; y = p[:, 1] + t * d[:, 1]; z = p[:, 2] + t * d[:, 2] - zv
        r = np.sqrt(x * x + y * y)
        k = np.where(r > rl, rl / np.where(r > 0, r, 1.0), 1.0)       # (beyond r_limit: a flat continuation along the radius)
        return z - sag(cx, cy, kx, ky, k * x, k * y)[0]

    with np.errstate(invalid="ignore", divide="ignore"):
        ta = (zv + zlo - p[:, 2]) / d[:, 2]
        tb = (zv + zhi - p[:, 2]) / d[:, 2]
    start = np.where(d[:, 2] > 0, ta, tb)
    end = np.where(d[:, 2] > 0, tb, ta)
    w = np.linspace(0.0, 1.0, scan)
    ts = start[:, None] + (end - start)[:, None] * w[None, :]
    fs = np.stack([f(ts[:, i]) for i in range(scan)], axis=1)
    flip = (fs[:, 1:] >= 0) != (fs[:, :1] >= 0)
    first = np.argmax(flip, axis=1)
    rows = np.arange(len(start))
    a, b = ts[rows, first].copy(), ts[rows, first + 1].copy()
    fa, fb = fs[rows, first].copy(), fs[rows, first + 1].copy()
    side = np.zeros(len(a), int)
    with np.errstate(invalid="ignore", divide="ignore"):
        for _ in range(200):                       # Illinois: a secant step that keeps the bracket
            c = (a * fb - b * fa) / (fb - fa)
            c = np.where(np.isfinite(c), c, 0.5 * (a + b))
            fc = f(c)
            left = (fc >= 0) == (fa >= 0)           # the root lies in [c, b]
            fb = np.where(left & (side == -1), 0.5 * fb, fb)
            fa = np.where(~left & (side == 1), 0.5 * fa, fa)
            side = np.where(left, -1, 1)
            a = np.where(left, c, a); fa = np.where(left, fc, fa)
            b = np.where(left, b, c); fb = np.where(left, fb, fc)
            if np.nanmax(np.minimum(np.abs(b - a), np.abs(fc))) < 1e-13:
                break
        t = np.where(np.abs(fa) < np.abs(fb), a, b)
    x = p[:, 0] + t * d[:, 0]; y = p[:, 1] + t * d[:, 1]
    bad = ~np.isfinite(t) | (x * x + y * y > rl * rl) | ~(np.abs(f(t)) <= 1e-9) | ~flip[rows, first]
    return np.where(bad, np.nan, t)


def event(p, d, zv, cx, cy, kx, ky, h, n_in, n_out, reflect, film=None, scan=513):
    """One event of n rays (p absolute, d unit) on a biconic: the dict of asphere_ref.event."""
    p = np.asarray(p, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    t = intersect(p, d, zv, cx, cy, kx, ky, h, scan)
    hit = p + t[:, None] * d
    x, y = hit[:, 0], hit[:, 1]
    r2 = x * x + y * y
    _, zx, zy = sag(cx, cy, kx, ky, x, y)
    n = np.stack([-zx, -zy, np.ones_like(x)], axis=1)
    n /= np.linalg.norm(n, axis=1)[:, None]
    dn = np.sum(d * n, axis=1)
    n = np.where((dn > 0)[:, None], -n, n)         # against the ray
    ci = np.abs(dn)
    eta = n_in / n_out
    k = 1.0 - eta * eta * (1.0 - ci * ci)
    ct = np.sqrt(np.maximum(k, 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = (n_in * ci - n_out * ct) / (n_in * ci + n_out * ct)
        rp = (n_out * ci - n_in * ct) / (n_out * ci + n_in * ct)
        Rb = np.where(k < 0, 1.0, 0.5 * (rs * rs + rp * rp))
        R = Rb if film is None else ar.film_reflectance(n_in, film[0], n_out, film[1], film[2], ci)
    if reflect:
        dout = d + 2.0 * ci[:, None] * n
        factor, bare = R, Rb
    else:
        dout = eta * d + (eta * ci - ct)[:, None] * n
        factor, bare = 1.0 - R, 1.0 - Rb
    fate = np.full(len(p), ALIVE)
    if not reflect:
        fate = np.where(k < 0, TIR, fate)
    fate = np.where(r2 > h * h, APERTURE, fate)
    fate = np.where(~np.isfinite(t), MISSED, fate)
    return dict(p=hit, d=dout, fate=fate, cos_i=ci, factor=factor, factor_bare=bare, rim=np.abs(np.sqrt(r2) - h))


def lens_geometry(lens):
    """asphere_ref.lens_geometry plus the biconic records: on, cx (1 / Rx, 0 for flat in x), kx, ky"""
    G = ar.lens_geometry(lens)
    b = lens.get("biconics")
    n = G["n"]
    G["bic_on"] = np.zeros(n, bool) if b is None else np.asarray(b["on"]) != 0
    rx = np.zeros(n) if b is None else np.asarray(b["radius_x"], np.float32).astype(np.float64)
    G["cx"] = np.where(rx != 0, 1.0 / np.where(rx != 0, rx, 1.0), 0.0)
    G["kx"] = np.zeros(n) if b is None else np.asarray(b["conic_x"], np.float64)
    G["ky"] = np.zeros(n) if b is None else np.asarray(b["conic_y"], np.float64)
    return G


def trace_path(lens, lam, i, j, sensor_xy, pupil_uv, mask=None, films=None):
    """asphere_ref.trace_path for a lens that may hold biconic records: the same returns -- n x 8 {exit point, unit
    direction, weight, alive}, the smallest incidence cosine and rim distance met, the events completed, the bare weight."""
    G = lens_geometry(lens)
    xy = np.asarray(sensor_xy, np.float32).astype(np.float64).reshape(-1, 2)
    uv = np.asarray(pupil_uv, np.float32).astype(np.float64).reshape(-1, 2)
    qx, qy = ar.pupil_disc(uv[:, 0], uv[:, 1])
    hp = G["h"][-1]
    vz = G["zv"][-1] - G["z_sensor"]
    p = np.stack([xy[:, 0], xy[:, 1], np.full(len(xy), G["z_sensor"])], axis=1)
    v = np.stack([hp * qx - xy[:, 0], hp * qy - xy[:, 1], np.full(len(xy), vz)], axis=1)
    d = v / np.linalg.norm(v, axis=1)[:, None]
    w = (np.pi * hp * hp / (vz * vz)) * d[:, 2] ** 4
    wb = w.copy()
    alive = np.ones(len(xy), bool)
    cmin = np.ones(len(xy)); rim = np.full(len(xy), np.inf); done = np.zeros(len(xy), int)
    ior = G["ior"][lam]
    for k, reflect, fwd in ar.sequence(G["n"], i, j):
        if k == G["stop"]:
            t = (G["zv"][k] - p[:, 2]) / d[:, 2]
            p = p + t[:, None] * d
            r2 = p[:, 0] ** 2 + p[:, 1] ** 2
            ok = r2 <= G["h"][k] ** 2
            rim = np.where(alive, np.minimum(rim, np.abs(np.sqrt(r2) - G["h"][k])), rim)
            if mask is not None:
                mh, mw = mask.shape
                fu = (p[:, 0] / G["h"][k] + 1.0) * 0.5 * mw; fv = (p[:, 1] / G["h"][k] + 1.0) * 0.5 * mh
                ix = np.clip(np.nan_to_num(fu).astype(int), 0, mw - 1); iy = np.clip(np.nan_to_num(fv).astype(int), 0, mh - 1)
                a = mask[iy, ix].astype(np.float64)
                w = w * a; wb = wb * a
                ok &= a > 0
            alive &= ok
            done += alive
            continue
        n_before = 1.0 if k == 0 else ior[k - 1] if k - 1 != G["stop"] else (1.0 if k - 2 < 0 else ior[k - 2])
        n_after = ior[k]
        n_in, n_out = (n_before, n_after) if fwd else (n_after, n_before)
        film = None
        if films is not None and films["thickness_nm"][k] > 0:
            film = (float(films["index"][lam, k]), float(films["thickness_nm"][k]), float(films["lambda_nm"][lam]))
        if G["bic_on"][k]:
            ev = event(p, d, G["zv"][k], G["cx"][k], G["c"][k], G["kx"][k], G["ky"][k], G["h"][k], n_in, n_out, reflect, film, scan=65)
        else:
            ev = ar.event(p, d, G["zv"][k], G["c"][k], G["kappa"][k], G["coef"][:, k], G["h"][k], n_in, n_out, reflect, film, scan=65)
        ok = ev["fate"] == ALIVE
        hit = ev["fate"] != MISSED
        cmin = np.where(alive & hit, np.minimum(cmin, np.nan_to_num(ev["cos_i"], nan=1.0)), cmin)
        rim = np.where(alive & hit, np.minimum(rim, np.nan_to_num(ev["rim"], nan=np.inf)), rim)
        p, d = ev["p"], ev["d"]
        w = w * ev["factor"]; wb = wb * ev["factor_bare"]
        alive &= ok
        done += alive
    out = np.zeros((len(xy), 8))
    out[:, 0:3] = p; out[:, 3:6] = d; out[:, 6] = np.where(alive, w, 0.0); out[:, 7] = alive
    return out, cmin, rim, done, np.where(alive, wb, 0.0)
