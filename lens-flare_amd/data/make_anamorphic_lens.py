"""Derives data/dgauss11_anamorphic.lens: dgauss11.lens behind an afocal pair of cylinders with power in x -- a
plano-concave cylinder in front, a convex-plano one behind it, both of a crown glass (n_d = 1.5168, V = 64.17; its C and F
indices synthesised by dgauss11.lens's own rule).  In y the four new faces are flat plates in a collimated beam: the y
meridian is dgauss11.lens.  In x the pair is a Galilean telescope: the air gap between the cylinders is SOLVED here, in
float64, by a paraxial trace of the x meridian through the thick elements, so that a collimated beam leaves the pair
collimated; the focal length in x is then the double Gauss's times the pair's angular magnification.

    python make_anamorphic_lens.py          writes dgauss11_anamorphic.lens beside this file
"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))

N_D, ABBE = 1.5168, 64.17
GLASS = (N_D - 0.3 * (N_D - 1.0) / ABBE, N_D, N_D + 0.7 * (N_D - 1.0) / ABBE)      # C, d, F
# (x-meridian radius, thickness, glass behind the face?, semi-aperture); the gap after the second face is solved
FRONT = [(0.0, 3.0, True, 38.0),        # plano ...
         (77.5, None, False, 38.0),     # ... concave cylinder; the air gap
         (103.4, 6.0, True, 18.0),      # convex ...
         (0.0, 2.0, False, 18.0)]       # ... plano cylinder; air to the double Gauss


def base_rows(text):
    rows = []
    for line in text.splitlines():
        line = line.split("#")[0].strip()
        if line and not line.startswith("sensor_width_mm"):
            rows.append([float(v) for v in line.split()])
    return rows


def trace(rows, col, y, u):
    """paraxial (height, slope) through rows (radius, thickness, index, ...): refraction then transfer at every row, the stop
    (index 0) a transfer only; returns (y, u) on the sensor and the heights at the rows"""
    n1 = 1.0
    for r in rows:
        n2 = r[2 + col]
        if n2 != 0.0:
            c = 0.0 if r[0] == 0.0 else 1.0 / r[0]
            u = c * (n1 - n2) / n2 * y + n1 / n2 * u
            n1 = n2
        y = y + r[1] * u
    return y, u


def image_scale(rows, col, stop):
    """where the chief ray of a collimated beam lands on the sensor, per radian of field angle"""
    ys = [trace(rows[:stop], col, *yu)[0] for yu in ((1.0, 0.0), (0.0, 1.0))]
    y0 = -ys[1] / ys[0]
    return y0 * trace(rows, col, 1.0, 0.0)[0] + trace(rows, col, 0.0, 1.0)[0]


def front_rows(gap, meridian):
    out = []
    for rx, t, glass, h in FRONT:
        idx = GLASS if glass else (1.0, 1.0, 1.0)
        out.append([rx if meridian == "x" else 0.0, gap if t is None else t, *idx, h])
    return out


def solve_gap():
    """the slope a collimated ray leaves the pair with is linear in the gap: two traces give its zero"""
    u = [trace(front_rows(g, "x"), 1, 1.0, 0.0)[1] for g in (0.0, 100.0)]
    return -u[0] * 100.0 / (u[1] - u[0])


def generate(base_text):
    base = base_rows(base_text)
    stop = 4 + [k for k, r in enumerate(base) if r[0] == 0.0 and r[2] == 0.0][0]
    gap = round(solve_gap(), 4)
    rx, ry = front_rows(gap, "x") + base, front_rows(gap, "y") + base
    sx, sy = image_scale(rx, 1, stop), image_scale(ry, 1, stop)
    fx, fy = trace(rx, 1, 1.0, 0.0), trace(ry, 1, 1.0, 0.0)
    fmt = lambda v: "1      " if v == 1.0 else "0      " if v == 0.0 else f"{v:.5f}"
    lines = [
        "# dgauss11.lens behind an AFOCAL PAIR OF CYLINDERS with power in x: the anamorphic lens of lf_set_lens_biconics.",
        "# Written by make_anamorphic_lens.py (beside this file), which derives every number below; not a published design.",
        "# Interfaces 0 - 3: a plano-concave cylinder (3 mm, second face Rx = +77.5) and, after an air gap, a convex-plano one",
        f"# (6 mm, first face Rx = +103.4) of a crown glass n_d = {N_D}, V = {ABBE} (C and F by dgauss11.lens's rule).  All four are",
        "# FLAT rows -- the y meridian is dgauss11.lens behind two plates -- and `biconic k Rx` gives interfaces 1 and 2 their",
        "# x-meridian radius: circular cylinders, z = cx x^2 / (1 + sqrt(1 - cx^2 x^2)), cx = 1 / Rx.",
        f"# The gap, {gap:.4f} mm, is solved in float64 by a paraxial trace of the x meridian through the thick elements (d line):",
        "# a collimated beam leaves the pair collimated, 103.4 / 77.5 times as wide.  A unit-height collimated ray then meets",
        f"# the sensor {abs(fx[0]):.1e} mm from the axis in x and {abs(fy[0]):.1e} mm in y.",
        f"# Paraxial image scales (mm per radian): x {sx:.4f}, y {sy:.4f}",
        f"# squeeze (scale_y / scale_x) = {sy / sx:.6f}",
        "# Interfaces 4 - 14 are dgauss11.lens's 0 - 10 (the stop is interface 9); rows, columns and the sensor as there.",
        "# 15 interfaces, 91 ghost pairs.  Bare glass, no coating line (films may be set on it: tests/test_gpu_biconics.py).",
        "sensor_width_mm 36.0",
    ]
    for r in front_rows(gap, "y"):
        lines.append(f"{r[0]:<9g} {r[1]:<7g} {fmt(r[2])} {fmt(r[3])} {fmt(r[4])} {r[5]:g}")
    body = [l for l in base_text.splitlines() if l.strip() and not l.startswith("#") and not l.startswith("sensor_width_mm")]
    lines += body
    for k, (r, _, _, _) in enumerate(FRONT):
        if r != 0.0:
            lines.append(f"biconic {k} {r:g}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = generate(open(os.path.join(HERE, "dgauss11.lens")).read())
    with open(os.path.join(HERE, "dgauss11_anamorphic.lens"), "w") as f:
        f.write(text)
    print(text, end="")
