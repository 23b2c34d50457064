"""A float64 tracer of a SENSOR path of the geometric lens (lf_set_sensor_ghosts) -- the reference of
tests/test_sensor_ghosts_cpu.py and tests/test_gpu_sensor_ghosts.py.  Built on tests/asphere_ref.py (event, lens_geometry,
pupil_disc) and, for biconic rows, tests/biconic_ref.py: unit directions, absolute z, bracketed intersections -- nothing of
the kernels' arithmetic.  The sensor's mirror is d.z -> -d.z at z = z_sensor with the rectangle test |x| <= half_w,
|y| <= half_h; the weight takes the reflectance as one factor."""
import numpy as np

import asphere_ref as ar
import biconic_ref as br

SENSOR = -1     # the interface index of the sensor's mirror in a sequence


def sequence(n, i):
    """(interface, reflect, forward) of the sensor path of interface i, in marching order; SENSOR stands for the mirror"""
    seq = [(k, False, False) for k in range(n - 1, i, -1)] + [(i, True, False)]
    seq += [(k, False, True) for k in range(i + 1, n)] + [(SENSOR, True, True)]
    seq += [(k, False, False) for k in range(n - 1, -1, -1)]
    return seq


def coded(n, i):
    """the sequence as lf_sensor_path_sequence writes it: interface | reflect << 8 | forward << 9, n for the sensor"""
    return np.array([(n if k == SENSOR else k) | int(r) << 8 | int(f) << 9 for k, r, f in sequence(n, i)], np.int32)


def rectangle(W, H, sensor_width_mm):
    """(half_w, half_h) in mm of a W x H frame on a sensor sensor_width_mm wide"""
    pitch = sensor_width_mm / W
    return 0.5 * W * pitch, 0.5 * H * pitch


def trace_sensor_path(lens, lam, i, sensor_xy, pupil_uv, half_w, half_h, reflectance=1.0, mask=None, films=None):
    """What asphere_ref.trace_path returns -- n x 8 {exit point, unit direction, weight, alive}, the smallest incidence cosine
    and rim distance met, the events completed, the bare weight -- plus, per ray, the distance from the rectangle's edge at
    the sensor's mirror (inf for a ray that never got there).  The rays start at the DEFAULT disc, as trace_path's do."""
    G = br.lens_geometry(lens)
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
    edge = np.full(len(xy), np.inf)
    ior = G["ior"][lam]
    for k, reflect, fwd in sequence(G["n"], i):
        if k == SENSOR:
            with np.errstate(invalid="ignore", divide="ignore"):
                t = (G["z_sensor"] - p[:, 2]) / d[:, 2]
            p = p + t[:, None] * d
            d = d * np.array([1.0, 1.0, -1.0])
            e = np.minimum(np.abs(half_w - np.abs(p[:, 0])), np.abs(half_h - np.abs(p[:, 1])))
            edge = np.where(alive, np.nan_to_num(e, nan=np.inf), edge)
            ok = (np.abs(p[:, 0]) <= half_w) & (np.abs(p[:, 1]) <= half_h)
            w = w * reflectance; wb = wb * reflectance
            alive &= ok
            done += alive
            continue
        if k == G["stop"]:
            with np.errstate(invalid="ignore", divide="ignore"):
                t = (G["zv"][k] - p[:, 2]) / d[:, 2]
            p = p + t[:, None] * d
            r2 = p[:, 0] ** 2 + p[:, 1] ** 2
            ok = r2 <= G["h"][k] ** 2
            rim = np.where(alive, np.minimum(rim, np.nan_to_num(np.abs(np.sqrt(r2) - G["h"][k]), nan=np.inf)), rim)
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
            ev = br.event(p, d, G["zv"][k], G["cx"][k], G["c"][k], G["kx"][k], G["ky"][k], G["h"][k], n_in, n_out, reflect, film, scan=65)
        else:
            ev = ar.event(p, d, G["zv"][k], G["c"][k], G["kappa"][k], G["coef"][:, k], G["h"][k], n_in, n_out, reflect, film, scan=65)
        ok = ev["fate"] == ar.ALIVE
        hit = ev["fate"] != ar.MISSED
        cmin = np.where(alive & hit, np.minimum(cmin, np.nan_to_num(ev["cos_i"], nan=1.0)), cmin)
        rim = np.where(alive & hit, np.minimum(rim, np.nan_to_num(ev["rim"], nan=np.inf)), rim)
        p, d = ev["p"], ev["d"]
        w = w * ev["factor"]; wb = wb * ev["factor_bare"]
        alive &= ok
        done += alive
    out = np.zeros((len(xy), 8))
    out[:, 0:3] = p; out[:, 3:6] = d; out[:, 6] = np.where(alive, w, 0.0); out[:, 7] = alive
    return out, cmin, rim, done, np.where(alive, wb, 0.0), edge


def excluded(cmin, rim, edge, bar, cos_min=0.05):
    """the rays a float32 comparison leaves out: within `bar` mm of an aperture rim or of the rectangle's edge, or with an
    incidence cosine <= cos_min somewhere on the way"""
    return (rim <= bar) | (edge <= bar) | (cmin <= cos_min)
