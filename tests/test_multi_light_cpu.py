"""CPU-only checks of the several-lights interface (lf_set_lights, lf_get_lights, lf_set_lights_from_flares): the
prototypes are in include/lensflare.h, the built library exports them, the Python wrapper exposes them and agrees with
the header about LF_MAX_LIGHTS.  What the calls compute is tests/test_gpu_multi_light.py's."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lf_set_lights", "lf_get_lights", "lf_set_lights_from_flares")


def _pkg():
    import __graft_entry__ as g
    return g.load_package()


def _header():
    return open(os.path.join(ROOT, "include", "lensflare.h")).read()


def test_prototypes_declared_and_exported():
    header = _header()
    lib = _pkg().load_library()
    for sym in NEW:
        assert re.search(r"^lf_status\s+%s\s*\(lf_ctx\*" % sym, header, re.M), sym
        assert hasattr(lib, sym), sym
        assert sym in _pkg().ABI_SYMBOLS
    # lf_set_sun and lf_set_sun_from_flares stay what they were
    assert re.search(r"^lf_status lf_set_sun\(lf_ctx\* ctx, const float dir\[3\], const float radiance\[3\],", header, re.M)
    assert "lf_status lf_set_sun_from_flares(lf_ctx* ctx, int flare, double efl_mm, float angular_radius);" in header


def test_wrapper_exposes_the_calls():
    pkg = _pkg()
    for name in ("set_lights", "lights", "set_lights_from_flares", "set_sun", "set_sun_from_flares"):
        assert callable(getattr(pkg.LensFlare, name)), name


def test_max_lights_agrees_with_the_header():
    m = re.search(r"^#define\s+LF_MAX_LIGHTS\s+(\d+)", _header(), re.M)
    assert m and int(m.group(1)) == _pkg().MAX_LIGHTS == 8
    # the test knob of the audit's test is documented where the others are
    assert '"cull_ignore_light"' in _header()
