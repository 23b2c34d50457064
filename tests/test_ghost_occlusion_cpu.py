"""Ghost occlusion without a device: the four entry points are declared and exported, the Python wrappers refuse bad arguments
before they reach the library, and lf_frame_plan's new field sits at the end and defaults to off in both host mirrors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lens-flare_amd", "host")
SYMBOLS = ["lf_set_ghost_occlusion", "lf_get_ghost_occlusion", "lf_get_ghost_occlusion_stats", "lf_ghost_ray_visibility"]


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def test_the_four_symbols_are_declared_and_exported():
    pkg = _pkg()
    header = open(os.path.join(ROOT, "include", "lensflare.h")).read()
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert re.search(r"lf_status\s+%s\s*\(\s*lf_ctx\s*\*" % s, header), s
        assert s in pkg.ABI_SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s)(*([C.c_void_p(0)] * 6)) == 1, s      # a NULL context: LF_ERR_INVALID, nothing dereferenced


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper reached the library ({name}) with arguments it should have refused")


def _bare(pkg):
    """a wrapper object with no context and no library behind it: whatever reaches the library fails the test"""
    lf = pkg.LensFlare.__new__(pkg.LensFlare)
    lf.lib, lf.ctx, lf._owned = _NoLibrary(), C.c_void_p(), False
    return lf


def test_the_wrappers_validate_their_arguments_without_a_device():
    pkg = _pkg()
    lf = _bare(pkg)
    for bad in (0.0, -0.001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            lf.set_ghost_occlusion(True, bad)
    for rays in (np.zeros(6), np.zeros((4, 5)), np.zeros((2, 3, 6)), [[0, 0, 0, 0, 0, 0.0]], [[0, 0, float("nan"), 0, 0, -1.0]],
                 [[float("inf"), 0, 0, 0, 0, -1.0]]):
        with pytest.raises(ValueError):
            lf.ghost_ray_visibility(rays)
    # ... and what is fine does reach it
    with pytest.raises(AssertionError):
        lf.set_ghost_occlusion(True, 0.001)
    with pytest.raises(AssertionError):
        lf.set_ghost_occlusion(False, -1.0)      # (off: the scale is not looked at, as in the library)
    with pytest.raises(AssertionError):
        lf.ghost_ray_visibility([[0, 0, 0, 0, 0, -1.0]])


PROBE = r"""
#include <cstddef>
#include <cstdio>
#include <cstring>
#include "lf_frame_sequence.h"
int main() {
  lf_frame_plan zeroed;
  std::memset(&zeroed, 0xff, sizeof(zeroed));
  std::memset(&zeroed, 0, sizeof(zeroed));          // what both mirrors do before they fill the plan in
  lf_frame_plan init = {};
  std::printf("%d %d %zu %zu %zu %zu\n", zeroed.ghost_occlusion, init.ghost_occlusion, offsetof(lf_frame_plan, ghost_occlusion),
              sizeof(int), sizeof(lf_frame_plan), offsetof(lf_frame_plan, geo_key));
  return 0;
}
"""


def test_the_frame_plans_field_is_last_and_defaults_to_off_in_both_mirrors(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", HOST, str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    zeroed, init, off, int_size, size, off_key = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert zeroed == 0 and init == 0
    assert off > off_key and off + int_size <= size and size - (off + int_size) < 8      # the last member (tail padding aside)
    # both mirrors zero the whole plan before they fill it in; the drop-in leaves the field off, the stand-alone mirror has a setter
    for name in ("pathtracer_amd.cpp", "lf_pathtracer.cpp"):
        text = open(os.path.join(HOST, name)).read()
        plan = text.index("lf_frame_plan plan;")
        assert re.search(r"memset\(&plan, 0, sizeof\(plan\)\);", text[plan:plan + 200]), name
        assert "plan.ghost_occlusion" in text[plan:], name
    dropin = open(os.path.join(HOST, "pathtracer_amd.cpp")).read()
    assert re.findall(r"plan\.ghost_occlusion\s*=\s*([^;]+);", dropin) == ["0"]
    mirror = open(os.path.join(HOST, "lf_pathtracer.cpp")).read()
    assert re.findall(r"plan\.ghost_occlusion\s*=\s*([^;]+);", mirror) == ["ghost_occlusion_ ? 1 : 0"]
    assert re.search(r"bool ghost_occlusion_ = false;", open(os.path.join(HOST, "lf_pathtracer.h")).read())
    # the one frame sequence installs the setting at every frame: on only with the march's ghosts, else off
    seq = open(os.path.join(HOST, "lf_frame_sequence.h")).read()
    assert re.search(r"lf_set_ghost_occlusion\(ctx, \(p->ghost_occlusion && p->ghosts == LF_FRAME_GHOSTS_MARCH\) \? 1 : 0,\s*p->world_per_mm\)", seq)
