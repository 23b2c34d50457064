"""Derives data/dgauss11_decentred.lens: dgauss11.lens with its SECOND ELEMENT -- the cemented doublet, interfaces 2 - 4 --
posed as a rigid group, a fraction of a millimetre off the axis and a fraction of a degree tilted about its front vertex, and
with ONE ROTATED CYLINDER on the front group: interface 1 becomes a weak toroid (its x-meridian radius shortened) whose axes
are turned about the optical axis.  The figures are chosen here, not taken from a published tolerance budget: of the size a
loose barrel and a badly seated element give.

A group's records follow the rule of lens_flare_amd.pose_group: the same R = Rx(ax) Ry(ay) Rz(az) on every interface and
t_k = d + (R - I) (0, 0, z_k - pivot_z) -- the faces of a tilted element need different records.

    python make_decentred_lens.py          writes dgauss11_decentred.lens beside this file
"""
import math
import os

HERE = os.path.dirname(os.path.abspath(__file__))

GROUP = (2, 4)                     # the cemented doublet: interfaces first .. last
GROUP_DECENTRE = (0.15, -0.10, 0.0)    # mm
GROUP_TILT = (0.20, -0.15, 0.0)        # degrees (ax, ay, az), about the group's front vertex
TOROID = 1                         # the interface that carries the rotated cylinder
TOROID_RX = 80.0                   # mm; the row's own radius (the y meridian) is 84.83
TOROID_AZ = 30.0                   # degrees about the optical axis


def rotation(ax, ay, az):
    a, b, g = (math.radians(v) for v in (ax, ay, az))
    ca, sa, cb, sb, cg, sg = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(g), math.sin(g)
    return [[cb * cg, -cb * sg, sb],
            [ca * sg + sa * sb * cg, ca * cg - sa * sb * sg, -sa * cb],
            [sa * sg - ca * sb * cg, sa * cg + ca * sb * sg, ca * cb]]


def generate(base_text):
    body = [l for l in base_text.splitlines() if l.strip() and not l.startswith("#") and not l.startswith("sensor_width_mm")]
    thick = [float(l.split()[1]) for l in body]
    z = [sum(thick[:k]) for k in range(len(body))]
    R = rotation(*GROUP_TILT)
    pivot = z[GROUP[0]]
    poses = []
    for k in range(GROUP[0], GROUP[1] + 1):
        lever = z[k] - pivot
        t = [GROUP_DECENTRE[i] + (R[i][2] - (1.0 if i == 2 else 0.0)) * lever for i in range(3)]
        poses.append((k, t, GROUP_TILT))
    lines = [
        "# dgauss11.lens with a DECENTRED, TILTED ELEMENT and a ROTATED CYLINDER: the posed lens of lf_set_lens_poses.",
        "# Written by make_decentred_lens.py (beside this file), which chooses every figure below; not a published tolerance budget.",
        f"# The second element, the cemented doublet (interfaces {GROUP[0]} - {GROUP[1]}), is posed as a rigid group: decentred by",
        f"# ({GROUP_DECENTRE[0]:g}, {GROUP_DECENTRE[1]:g}, {GROUP_DECENTRE[2]:g}) mm and tilted by (ax, ay, az) = ({GROUP_TILT[0]:g}, {GROUP_TILT[1]:g}, {GROUP_TILT[2]:g}) degrees about its front vertex",
        "# (pose_group's rule: the same rotation on every face, t_k = d + (R - I) (0, 0, z_k - pivot_z)).",
        f"# Interface {TOROID} is a weak toroid, Rx = {TOROID_RX:g} against the row's {body[TOROID].split()[0]} in y (`biconic`), its axes turned by az = {TOROID_AZ:g}",
        "# degrees about the optical axis (`pose`): a rotated cylinder on the front group.",
        "# Rows, columns and the sensor are dgauss11.lens's; 11 interfaces, 45 ghost pairs.  With the pose lines removed the lens",
        "# still carries the biconic record, so both are marched by the Newton march.  Bare glass, no coating line (films may be",
        "# set on it: tests/test_gpu_poses.py).",
        "sensor_width_mm 36.0",
    ]
    lines += body
    lines.append(f"biconic {TOROID} {TOROID_RX:g}")
    lines.append(f"pose {TOROID} 0 0 0 0 0 {TOROID_AZ:g}")
    for k, t, a in poses:
        lines.append(f"pose {k} {t[0]:.7g} {t[1]:.7g} {t[2]:.7g} {a[0]:g} {a[1]:g} {a[2]:g}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = generate(open(os.path.join(HERE, "dgauss11.lens")).read())
    with open(os.path.join(HERE, "dgauss11_decentred.lens"), "w") as f:
        f.write(text)
    print(text, end="")
