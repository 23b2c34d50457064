"""A float64 numpy tracer for POSED interfaces (decentred, tilted, rotated: lf_set_lens_poses) -- the reference of
tests/test_poses_cpu.py and tests/test_gpu_poses.py, written independently of the kernels' event (lens-flare_amd/csrc/lf_pose.h):

  * the ray STAYS in lens coordinates and the surface moves: the interface is the zero set of
        g(P) = q_z - sag(q_x, q_y),   q = R^T (P - V - t),   R = Rx(ax) Ry(ay) Rz(az)
    (the kernel carries the ray into the surface's frame, runs its un-posed event there and carries the result back);
  * the root of g along the ray is BRACKETED between the two planes that bound the sag over the clear disc (planes of the
    surface's own frame, met by the lens-frame ray), the span scanned for its first change of sign, that interval bisected
    and the root polished by two Newton steps on g -- the kernel starts from a quadric's root and only ever runs Newton;
  * the normal is the gradient of g in lens coordinates, R (-z_x, -z_y, 1);
  * rays carry UNIT directions and absolute z; Snell's law and the mirror are the unit-direction vector forms.

The sags are tests/asphere_ref.py's (a surface of revolution) and tests/biconic_ref.py's (a biconic); the lens geometry, the
pupil map and the films are theirs too.  Fates as there: 0 alive, 1 missed, 2 outside the clear aperture, 3 totally
reflected, 4 blocked by the stop mask."""
import numpy as np

import asphere_ref as ar
import biconic_ref as br
from asphere_ref import ALIVE, MISSED, APERTURE, TIR, CLIPPED  # noqa: F401


def rotation(tilt_deg):
    """R = Rx(ax) Ry(ay) Rz(az), right-handed, degrees -- built as the product of the three elementary matrices"""
    ax, ay, az = np.deg2rad(np.asarray(tilt_deg, np.float64))
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(ax), -np.sin(ax)], [0.0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0.0, np.sin(ay)], [0.0, 1.0, 0.0], [-np.sin(ay), 0.0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0.0], [np.sin(az), np.cos(az), 0.0], [0.0, 0.0, 1.0]])
    return rx @ ry @ rz


def surface(kind, **kw):
    """the description of an un-posed surface: kind "asph" (c, kappa, coef) or "bic" (cx, cy, kx, ky)"""
    if kind == "asph":
        return dict(kind="asph", c=float(kw["c"]), kappa=float(kw.get("kappa", 0.0)),
                    coef=np.asarray(kw.get("coef", ()), np.float64).ravel())
    return dict(kind="bic", cx=float(kw["cx"]), cy=float(kw["cy"]), kx=float(kw.get("kx", 0.0)), ky=float(kw.get("ky", 0.0)))


def _sag(S, x, y):
    """z, z_x, z_y of the un-posed surface"""
    if S["kind"] == "asph":
        z, zp = ar.sag(S["c"], S["kappa"], S["coef"], x * x + y * y)
        return z, 2.0 * zp * x, 2.0 * zp * y
    return br.sag(S["cx"], S["cy"], S["kx"], S["ky"], x, y)


def _r_limit(S, h):
    if S["kind"] == "asph":
        return ar.r_limit(S["c"], S["kappa"], h)
    return br.r_limit(S["cx"], S["cy"], S["kx"], S["ky"], h)


def intersect(p, d, V, S, h, R, t0, scan=513):
    """ray parameter of the first crossing of p + s d with the posed surface; NaN where there is none"""
    rl = _r_limit(S, h)
    g1 = np.linspace(-rl, rl, 257)
    gx, gy = np.meshgrid(g1, g1)
    inside = gx * gx + gy * gy <= rl * rl
    zs = _sag(S, gx[inside], gy[inside])[0]
    zlo, zhi = float(np.min(zs)) - 1e-9, float(np.max(zs)) + 1e-9
    origin = np.asarray(V, np.float64) + np.asarray(t0, np.float64)

    def local(s):
        return (p + s[:, None] * d - origin) @ R          # rows: R^T (P - V - t)

    def g(s):
        q = local(s)
        r = np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2)
        k = np.where(r > rl, rl / np.where(r > 0, r, 1.0), 1.0)      # (beyond r_limit: a flat continuation along the radius)
        return q[:, 2] - _sag(S, k * q[:, 0], k * q[:, 1])[0]

    a = ((p - origin) @ R)[:, 2]
    b = (d @ R)[:, 2]                                      # the local K'_z
    with np.errstate(invalid="ignore", divide="ignore"):
        ta = (zlo - a) / b
        tb = (zhi - a) / b
    start = np.where(b > 0, ta, tb)
    end = np.where(b > 0, tb, ta)
    w = np.linspace(0.0, 1.0, scan)
    ts = start[:, None] + (end - start)[:, None] * w[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        fs = np.stack([g(ts[:, i]) for i in range(scan)], axis=1)
        flip = (fs[:, 1:] >= 0) != (fs[:, :1] >= 0)
        first = np.argmax(flip, axis=1)
        rows = np.arange(len(start))
        lo, hi = ts[rows, first].copy(), ts[rows, first + 1].copy()
        up = fs[rows, first] < 0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            below = (g(mid) < 0) == up
            lo = np.where(below, mid, lo); hi = np.where(below, hi, mid)
            if np.nanmax(np.abs(hi - lo)) < 1e-13:
                break
        s = 0.5 * (lo + hi)
        for _ in range(2):                                 # polish on the true surface: Newton on g with its gradient
            q = local(s)
            z, zx, zy = _sag(S, q[:, 0], q[:, 1])
            grad = np.stack([-zx, -zy, np.ones_like(zx)], axis=1) @ R.T          # R (-z_x, -z_y, 1)
            gp = np.sum(grad * d, axis=1)
            s = np.where(np.isfinite(z) & np.isfinite(gp) & (gp != 0), s - (q[:, 2] - z) / gp, s)
        q = local(s)
        bad = ~np.isfinite(s) | (q[:, 0] ** 2 + q[:, 1] ** 2 > rl * rl) | ~(np.abs(g(s)) <= 1e-9) | ~flip[rows, first]
    return np.where(bad, np.nan, s)


def event(p, d, V, S, h, decentre, tilt_deg, n_in, n_out, reflect, forward, film=None, scan=513):
    """One event of n rays (p absolute, d unit) on the posed surface S (vertex nominally at V = (0, 0, zv)): the dict of
    asphere_ref.event, plus q, the hit in the surface's frame.  forward: the row's direction of travel is +z."""
    p = np.asarray(p, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    R = rotation(tilt_deg)
    t0 = np.asarray(decentre, np.float64)
    s = intersect(p, d, V, S, h, R, t0, scan)
    hit = p + s[:, None] * d
    q = (hit - np.asarray(V, np.float64) - t0) @ R
    r2 = q[:, 0] ** 2 + q[:, 1] ** 2                      # the rim moves with the glass
    _, zx, zy = _sag(S, q[:, 0], q[:, 1])
    n = np.stack([-zx, -zy, np.ones_like(zx)], axis=1) @ R.T
    n /= np.linalg.norm(n, axis=1)[:, None]
    dn = np.sum(d * n, axis=1)
    n = np.where((dn > 0)[:, None], -n, n)                 # against the ray
    ci = np.abs(dn)
    eta = n_in / n_out
    k = 1.0 - eta * eta * (1.0 - ci * ci)
    ct = np.sqrt(np.maximum(k, 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = (n_in * ci - n_out * ct) / (n_in * ci + n_out * ct)
        rp = (n_out * ci - n_in * ct) / (n_out * ci + n_in * ct)
        Rb = np.where(k < 0, 1.0, 0.5 * (rs * rs + rp * rp))
        Rf = Rb if film is None else ar.film_reflectance(n_in, film[0], n_out, film[1], film[2], ci)
    if reflect:
        dout = d + 2.0 * ci[:, None] * n
        factor, bare = Rf, Rb
    else:
        dout = eta * d + (eta * ci - ct)[:, None] * n
        factor, bare = 1.0 - Rf, 1.0 - Rb
    fate = np.full(len(p), ALIVE)
    if not reflect:
        fate = np.where(k < 0, TIR, fate)
    fate = np.where(r2 > h * h, APERTURE, fate)
    fate = np.where(~np.isfinite(s), MISSED, fate)
    towards = (d @ R)[:, 2] * (1.0 if forward else -1.0) > 0          # the ray meets the surface from the row's side
    fate = np.where(~towards, MISSED, fate)
    return dict(p=hit, d=dout, q=q, fate=fate, cos_i=ci, factor=factor, factor_bare=bare, rim=np.abs(np.sqrt(r2) - h),
                towards_margin=np.abs((d @ R)[:, 2]))


def lens_geometry(lens):
    """biconic_ref.lens_geometry plus the pose records: pose_on, pose_t (n x 3), pose_a (n x 3 degrees)"""
    G = br.lens_geometry(lens)
    n = G["n"]
    po = lens.get("poses")
    G["pose_on"] = np.zeros(n, bool) if po is None else np.asarray(po["on"]) != 0
    G["pose_t"] = np.zeros((n, 3)) if po is None else np.asarray(po["decentre"], np.float32).astype(np.float64).reshape(n, 3)
    G["pose_a"] = np.zeros((n, 3)) if po is None else np.asarray(po["tilt_deg"], np.float32).astype(np.float64).reshape(n, 3)
    return G


def surface_of(G, k):
    """interface k of a lens geometry as `surface` describes it (a sphere or a plane: a surface of revolution)"""
    if G["bic_on"][k]:
        return surface("bic", cx=G["cx"][k], cy=G["c"][k], kx=G["kx"][k], ky=G["ky"][k])
    return surface("asph", c=G["c"][k], kappa=G["kappa"][k], coef=G["coef"][:, k])


def trace_path(lens, lam, i, j, sensor_xy, pupil_uv, mask=None, films=None, scan=65):
    """biconic_ref.trace_path for a lens that may hold pose records: the same returns -- n x 8 {exit point, unit direction,
    weight, alive}, the smallest incidence cosine and rim distance met, the events completed, the bare weight."""
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
        if G["pose_on"][k]:
            ev = event(p, d, (0.0, 0.0, G["zv"][k]), surface_of(G, k), G["h"][k], G["pose_t"][k], G["pose_a"][k], n_in, n_out,
                       reflect, fwd, film, scan=scan)
        elif G["bic_on"][k]:
            ev = br.event(p, d, G["zv"][k], G["cx"][k], G["c"][k], G["kx"][k], G["ky"][k], G["h"][k], n_in, n_out, reflect, film, scan=scan)
        else:
            ev = ar.event(p, d, G["zv"][k], G["c"][k], G["kappa"][k], G["coef"][:, k], G["h"][k], n_in, n_out, reflect, film, scan=scan)
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
