"""A float64 tracer of a SENSOR path through a lens that may hold pose records (lf_set_sensor_ghost_surfaces) -- the reference
of tests/test_sensor_poses_cpu.py and tests/test_gpu_sensor_poses.py.  It is tests/sensor_ghost_ref.py's trace_sensor_path
with ONE change: a row whose interface has a pose record goes through tests/pose_ref.py's event, which moves the surface and
leaves the ray in lens coordinates (the kernels carry the ray into the surface's frame: lens-flare_amd/csrc/lf_pose.h) -- with
the row's own direction of travel, on each of the up to three crossings.  Geometry from pose_ref.lens_geometry and
pose_ref.surface_of; nothing of the kernels' arithmetic."""
import numpy as np

import asphere_ref as ar
import biconic_ref as br
import pose_ref as pr
import sensor_ghost_ref as sg
from sensor_ghost_ref import SENSOR, sequence, rectangle, excluded  # noqa: F401


def trace_sensor_path(lens, lam, i, sensor_xy, pupil_uv, half_w, half_h, reflectance=1.0, mask=None, films=None):
    """What sensor_ghost_ref.trace_sensor_path returns -- n x 8 {exit point, unit direction, weight, alive}, the smallest
    incidence cosine and rim distance met, the events completed, the bare weight, the distance from the rectangle's edge at
    the sensor's mirror -- plus the smallest towards_margin |K'_z| met on a posed row (inf where the ray met none).  The
    rays start at the DEFAULT disc: the centred rear element's clear aperture at its nominal vertex plane."""
    G = pr.lens_geometry(lens)
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
    towards = np.full(len(xy), np.inf)
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
        if G["pose_on"][k]:          # the one change: the surface moves, the ray stays (pose_ref.event), the row's own direction
            ev = pr.event(p, d, (0.0, 0.0, G["zv"][k]), pr.surface_of(G, k), G["h"][k], G["pose_t"][k], G["pose_a"][k], n_in, n_out,
                          reflect, fwd, film, scan=65)
            towards = np.where(alive, np.minimum(towards, np.nan_to_num(ev["towards_margin"], nan=0.0)), towards)
        elif G["bic_on"][k]:
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
    return out, cmin, rim, done, np.where(alive, wb, 0.0), edge, towards


def left_out(cmin, rim, edge, towards, bar, cos_min=0.05):
    """sensor_ghost_ref.excluded, plus the rays whose local K'_z on a posed row is within `bar` of changing sign"""
    return sg.excluded(cmin, rim, edge, bar, cos_min) | (towards <= bar)
