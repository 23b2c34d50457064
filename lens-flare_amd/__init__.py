"""lens_flare_amd: Python plumbing over the C ABI of liblensflare_hip.so (include/lensflare.h).

The product is the C-ABI library (hand-written gfx950 kernels); the C++ host shim that mirrors the
reference's PathTracer surface lives in host/.  This module only binds the same entry points with
ctypes so tests/ and bench.py can drive them; it contains no compute and no fallback: if the
library (or a GPU) is missing every call fails loudly.

The directory is named `lens-flare_amd` (not importable by name); load it with
`__graft_entry__.load_package()` which registers it as `lens_flare_amd`.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# LF_LIB: experiments only (profiles/ab_*.sh time alternative builds of the same library)
LIB_PATH = os.environ.get("LF_LIB") or os.path.join(HERE, "liblensflare_hip.so")
DATA = os.path.join(HERE, "data")

STATUS = {0: "LF_OK", 1: "LF_ERR_INVALID", 2: "LF_ERR_NO_DEVICE", 3: "LF_ERR_HIP",
          4: "LF_ERR_STATE", 5: "LF_ERR_OOM", 6: "LF_ERR_UNSUPPORTED"}
APERTURE_STARBURST, APERTURE_GHOST = 0, 1
MAX_LIGHTS = 8   # LF_MAX_LIGHTS: lights one launch of the geometric march follows (set_lights)
SAMPLE_BUFFER, GHOST_BUFFER, STARBURST_BUFFER, SCENE_BUFFER = 0, 1, 2, 3
# the sampling specification's defaults (lf_internal.h): 64 x 64 pupil sub-cells, wave tiles with columns 8 apart
DEFAULT_SUBCELL_BITS, DEFAULT_TILE_STRIDE = 6, 8

# every symbol include/lensflare.h declares
ABI_SYMBOLS = [
    "lf_create", "lf_destroy", "lf_last_error", "lf_abi_version", "lf_set_stream", "lf_synchronize",
    "lf_set_frame", "lf_set_band", "lf_set_row_interleave", "lf_set_block_deal", "lf_set_params", "lf_set_aperture", "lf_get_aperture_stats",
    "lf_set_paraxial_lens", "lf_set_camera", "lf_find_sun_pos", "lf_set_flares", "lf_get_flares",
    "lf_set_jitter_mt19937", "lf_set_jitter_counter", "lf_set_scene_term", "lf_set_scene",
    "lf_set_sampling", "lf_scene_bounds", "lf_set_scene_lights", "lf_set_light_samples", "lf_set_environment_map",
    "lf_set_direct_hemisphere_sample", "lf_collada_check", "lf_render_scene_term",
    "lf_generate_ghost_buffer", "lf_render_flare_layer", "lf_read_tile", "lf_read_pixel",
    "lf_write_to_framebuffer", "lf_save_image_rgba", "lf_device_buffer", "lf_set_lens", "lf_set_lambda_rgb", "lf_set_sun",
    "lf_set_lights", "lf_get_lights", "lf_set_lights_from_flares",
    "lf_set_lights_ex", "lf_get_lights_ex", "lf_validate_light", "lf_light_lobe_factor", "lf_ghost_ray_light_factors",
    "lf_set_lights_from_scene",
    "lf_set_lights_geom", "lf_get_lights_geom", "lf_validate_light_geom", "lf_light_geom_factor", "lf_area_light_pretest",
    "lf_ghost_shadow_reach_geom", "lf_area_light_cull_cone", "lf_set_lights_from_scene_ex",
    "lf_set_ghost_occlusion", "lf_get_ghost_occlusion", "lf_get_ghost_occlusion_stats", "lf_ghost_ray_visibility",
    "lf_set_ghost_occlusion_reach", "lf_get_ghost_occlusion_reach", "lf_ghost_shadow_reach", "lf_ghost_ray_light_visibility",
    "lf_set_flare_occlusion", "lf_get_flare_occlusion", "lf_get_flare_visibility", "lf_flare_shadow_samples", "lf_flare_shadow_rays",
    "lf_set_sun_from_flares", "lf_paraxial_efl", "lf_paraxial_image_scale", "lf_set_ghost_pairs", "lf_set_pupil_subcells", "lf_set_tile_stride", "lf_trace_ghosts", "lf_set_march_culling", "lf_get_cull_info", "lf_get_cull_table", "lf_get_cull_started_fraction", "lf_get_cull_reason", "lf_set_cull_audit", "lf_get_cull_audit", "lf_test_knob", "lf_comm_share_cull", "lf_set_cull_share", "lf_cull_prepare", "lf_cull_table_view", "lf_cull_commit", "lf_get_march_fix_bits", "lf_generate_lens_rays", "lf_get_counters", "lf_reset_counters", "lf_get_executed_events", "lf_get_march_stats", "lf_native_sqrt", "lf_native_rcp", "lf_set_starburst_spectrum", "lf_load_collada", "lf_march_tables",
    "lf_timing_enable", "lf_timing_reset", "lf_timing_get",
    "lf_clear_ghost_buffer", "lf_draw_ghost", "lf_rasterize_textured_triangle", "lf_fill_textured_pixel",
    "lf_shift_vertex", "lf_compute_phase", "lf_irradiance_falloff", "lf_scene_trace_ray", "lf_scene_shade",
    "lf_load_lens_file", "lf_get_lens_info", "lf_set_lens_coatings", "lf_get_lens_coatings", "lf_coating_reflectance",
    "lf_set_lens_coating_stacks", "lf_get_lens_coating_stacks", "lf_coating_stack_reflectance",
    "lf_set_lens_aspheres", "lf_get_lens_aspheres", "lf_asphere_sag", "lf_asphere_event", "lf_asphere_events", "lf_march_path_rays",
    "lf_set_lens_biconics", "lf_get_lens_biconics", "lf_get_lens_meridian_scales", "lf_biconic_sag", "lf_biconic_event", "lf_biconic_events",
    "lf_set_lens_poses", "lf_get_lens_poses", "lf_pose_event", "lf_pose_events",
    "lf_set_sensor_reflectance", "lf_get_sensor_reflectance", "lf_set_sensor_ghosts", "lf_get_sensor_ghosts",
    "lf_march_sensor_path_rays", "lf_sensor_path_sequence", "lf_sensor_mirror_event", "lf_get_sensor_ghost_stats",
    "lf_set_sensor_ghost_surfaces", "lf_get_sensor_ghost_surfaces",
    "lf_set_mask_filter", "lf_get_mask_filter", "lf_mask_lookup",
    "lf_set_pupil_target", "lf_get_pupil_target", "lf_aim_at_exit_pupil", "lf_paraxial_exit_pupil", "lf_set_ghost_accumulate",
    "lf_set_lens_camera", "lf_get_lens_camera", "lf_set_lens_camera_aim", "lf_set_lens_camera_surfaces", "lf_get_lens_camera_surfaces",
    "lf_lens_camera_samples", "lf_paraxial_entrance_pupil", "lf_focus_lens", "lf_focus_lens_from_pupil",
    "lf_get_scene_counters", "lf_reset_scene_counters", "lf_set_flare_arithmetic",
    "lf_comm_get_unique_id", "lf_comm_init_rank", "lf_comm_gather", "lf_comm_gather_async", "lf_comm_wait",
    "lf_comm_destroy", "lf_comm_available", "lf_comm_info", "lf_comm_test", "lf_comm_abort",
    "lf_comm_set_exchange_precision", "lf_comm_poison", "lf_comm_is_poisoned", "lf_comm_exchange_plan",
    "lf_group_create", "lf_group_destroy", "lf_group_size", "lf_group_ctx", "lf_group_last_error",
    "lf_group_set_frame", "lf_group_for_each", "lf_group_gather", "lf_group_share_cull", "lf_group_set_block_deal",
]


def test_knob_default(name, value):
    """TEST HOOK: lf_test_knob(NULL, ...) -- the knob's value for every context created from now on (0: none)"""
    st = load_library().lf_test_knob(None, name.encode(), C.c_double(float(value)))
    if st != 0:
        raise LensFlareError(st, "lf_test_knob")


test_knob_default.__test__ = False      # (not a test, whatever pytest thinks of the name)


def paraxial_exit_pupil(lens, lam=None):
    """(z_mm, magnification) of the paraxial image of the stop through the rear group (host arithmetic)."""
    lib = load_library()
    ior = np.ascontiguousarray(lens["ior"], np.float32)
    lam = ior.shape[0] // 2 if lam is None else lam
    r = np.ascontiguousarray(lens["radius"], np.float32)
    t = np.ascontiguousarray(lens["thickness"], np.float32)
    row = np.ascontiguousarray(ior[lam], np.float32)
    z, m = C.c_double(), C.c_double()
    st = lib.lf_paraxial_exit_pupil(int(lens["n"]), int(lens["stop"]), _fp(r, C.c_float), _fp(t, C.c_float),
                                    _fp(row, C.c_float), C.byref(z), C.byref(m))
    if st != 0:
        raise LensFlareError(st, "lf_paraxial_exit_pupil")
    return z.value, m.value


def paraxial_entrance_pupil(lens, lam=None):
    """(z_mm, magnification) of the paraxial image of the stop through the front group (host arithmetic)."""
    lib = load_library()
    ior = np.ascontiguousarray(lens["ior"], np.float32)
    lam = ior.shape[0] // 2 if lam is None else lam
    r = np.ascontiguousarray(lens["radius"], np.float32)
    t = np.ascontiguousarray(lens["thickness"], np.float32)
    row = np.ascontiguousarray(ior[lam], np.float32)
    z, m = C.c_double(), C.c_double()
    st = lib.lf_paraxial_entrance_pupil(int(lens["n"]), int(lens["stop"]), _fp(r, C.c_float), _fp(t, C.c_float),
                                        _fp(row, C.c_float), C.byref(z), C.byref(m))
    if st != 0:
        raise LensFlareError(st, "lf_paraxial_entrance_pupil")
    return z.value, m.value


class LensFlareError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS.get(status, status)}: {msg}")
        self.status = status


class ApertureStats(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("min_x", C.c_int), ("min_y", C.c_int),
                ("max_x", C.c_int), ("max_y", C.c_int), ("total_value", C.c_double)]


class ColladaCamera(C.Structure):
    _fields_ = [("present", C.c_int), ("hfov", C.c_double), ("vfov", C.c_double), ("nclip", C.c_double),
                ("fclip", C.c_double), ("pos", C.c_double * 3), ("dir", C.c_double * 3), ("up", C.c_double * 3)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rays_launched", "surface_events", "rays_clipped_stop",
                                          "rays_vignetted", "rays_tir", "rays_reached_scene",
                                          "rays_hit_light")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


_lib = None


def load_library():
    """dlopen the in-tree library.  Raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            # never built lazily: a build started from a process that has touched the GPU (or from
            # N torchrun ranks at once, or under rocprofv3) is exactly what must not happen
            raise FileNotFoundError(f"{LIB_PATH} is missing: run __graft_entry__.build() "
                                    "(make -C lens-flare_amd) before any GPU work")
        lib = C.CDLL(LIB_PATH)
        lib.lf_last_error.restype = C.c_char_p
        lib.lf_last_error.argtypes = [C.c_void_p]
        _lib = lib
    return _lib


def _fp(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def load_aperture_png(path):
    """An aperture PNG -> float texels exactly as CameraApertureTexture::init derives them
    (camera.h:39-63: lodepng RGBA8, red byte x float(1/255), CGL/src/color.cpp:16-21).  The decode is
    host plumbing (the ABI takes texels); names without a directory are looked up in data/."""
    from PIL import Image
    if not os.path.isabs(path) and not os.path.exists(path):
        path = os.path.join(DATA, path)
    red = np.ascontiguousarray(np.asarray(Image.open(path).convert("RGBA"))[:, :, 0])
    return red.astype(np.float32) * np.float32(1.0 / 255.0)


def load_lens_file(path):
    """Parse a .lens prescription (see data/dgauss11.lens) -> dict of float32 arrays."""
    if not os.path.isabs(path) and not os.path.exists(path):
        path = os.path.join(DATA, path)
    rows, sensor_w, lambda_nm, coats, layers, asphs, bics, sens, poses = [], 36.0, None, [], [], [], [], None, []
    for line in open(path):
        line = line.split("#")[0].strip()
        if not line:
            continue
        t = line.split()
        if t[0] == "sensor_width_mm":
            sensor_w = float(t[1])
            continue
        if t[0] == "sensor_reflectance":   # sensor_reflectance r_1 .. r_L | r  (lf_set_sensor_reflectance)
            if sens is not None or len(t) < 2:
                raise ValueError(f"{path}: a sensor_reflectance line is `sensor_reflectance r_1 .. r_L` or `sensor_reflectance r` (once)")
            sens = [float(v) for v in t[1:]]
            continue
        if t[0] == "lambda_nm":      # the wavelengths of the index columns (spectral prescriptions)
            lambda_nm = [float(v) for v in t[1:]]
            continue
        if t[0] == "coating":        # coating k thickness_nm m_1 .. m_L | m  (lf_set_lens_coatings)
            coats.append((int(t[1]), float(t[2]), [float(v) for v in t[3:]]))
            continue
        if t[0] == "layer":          # layer k thickness_nm m_1 .. m_L | m  (appends to interface k's stack, scene side first)
            layers.append((int(t[1]), float(t[2]), [float(v) for v in t[3:]]))
            continue
        if t[0] == "asphere":        # asphere k kappa [A4 [A6 .. A14]]  (lf_set_lens_aspheres)
            if len(t) < 3 or len(t) > 3 + MAX_ASPH_COEF:
                raise ValueError(f"{path}: an asphere line is `asphere k kappa [A4 [A6 .. A14]]`")
            asphs.append((int(t[1]), float(t[2]), [float(v) for v in t[3:]]))
            continue
        if t[0] == "biconic":        # biconic k Rx [kx [ky]]  (lf_set_lens_biconics; Rx = 0: flat in x)
            if len(t) < 3 or len(t) > 5:
                raise ValueError(f"{path}: a biconic line is `biconic k Rx [kx [ky]]`")
            bics.append((int(t[1]), [float(v) for v in t[2:]]))
            continue
        if t[0] == "pose":           # pose k dx dy dz ax ay az  (lf_set_lens_poses; mm and degrees)
            if len(t) != 8:
                raise ValueError(f"{path}: a pose line is `pose k dx dy dz ax ay az`")
            poses.append((int(t[1]), [float(v) for v in t[2:]]))
            continue
        rows.append([float(v) for v in t])
    rows = np.array(rows, np.float64)
    n = len(rows)
    stop = [k for k in range(n) if rows[k, 0] == 0 and rows[k, 3] == 0]
    ior = rows[:, 2:-1].T.copy()  # n_lambda x n
    if stop:
        ior[:, stop[0]] = 1.0
    lens = dict(n=n, stop=stop[0] if stop else -1, radius=rows[:, 0].astype(np.float32),
                thickness=rows[:, 1].astype(np.float32), ior=ior.astype(np.float32),
                semi_aperture=rows[:, -1].astype(np.float32), sensor_width_mm=float(sensor_w))
    if sens is not None:
        if len(sens) not in (1, ior.shape[0]) or not all(0.0 <= v <= 1.0 for v in sens):
            raise ValueError(f"{path}: sensor_reflectance takes one value in [0, 1], or one per index column")
        lens["sensor_reflectance"] = np.array(sens if len(sens) > 1 else sens * ior.shape[0], np.float32)
    if asphs:
        conic = np.zeros(n, np.float32)
        coef = np.zeros((MAX_ASPH_COEF, n), np.float32)
        seen = set()
        for k, kappa, a in asphs:
            if not 0 <= k < n or k in seen:
                raise ValueError(f"{path}: bad asphere line for interface {k}")
            seen.add(k)
            conic[k] = kappa
            coef[:len(a), k] = a
        lens["aspheres"] = dict(conic=conic, coef=coef)
    if bics:
        on = np.zeros(n, np.int32)
        rec = np.zeros((3, n), np.float32)       # Rx, kx, ky
        for k, v in bics:
            if not 0 <= k < n or on[k]:
                raise ValueError(f"{path}: bad biconic line for interface {k}")
            if k == lens["stop"]:
                raise ValueError(f"{path}: a biconic line on the stop (interface {k})")
            if "aspheres" in lens and (lens["aspheres"]["conic"][k] != 0 or lens["aspheres"]["coef"][:, k].any()):
                raise ValueError(f"{path}: interface {k} has an asphere line and a biconic line")
            on[k] = 1
            rec[:len(v), k] = v
        lens["biconics"] = dict(on=on, radius_x=rec[0].copy(), conic_x=rec[1].copy(), conic_y=rec[2].copy())
    if poses:
        on = np.zeros(n, np.int32)
        rec = np.zeros((n, 6), np.float32)       # dx, dy, dz, ax, ay, az
        for k, v in poses:
            if not 0 <= k < n or on[k]:
                raise ValueError(f"{path}: bad pose line for interface {k}")
            if k == lens["stop"]:
                raise ValueError(f"{path}: a pose line on the stop (interface {k})")
            if not np.all(np.isfinite(v)) or abs(v[3]) > 30 or abs(v[4]) > 30 or abs(v[5]) > 180:
                raise ValueError(f"{path}: interface {k}: |ax|, |ay| <= 30 and |az| <= 180 degrees, every value finite")
            on[k] = 1
            rec[k] = v
        lens["poses"] = dict(on=on, decentre=rec[:, :3].copy(), tilt_deg=rec[:, 3:].copy())
    if lambda_nm is not None:
        if len(lambda_nm) != ior.shape[0]:
            raise ValueError(f"{path}: lambda_nm lists {len(lambda_nm)} wavelengths for {ior.shape[0]} index columns")
        lens["lambda_nm"] = np.array(lambda_nm, np.float64)
    if coats:
        if lambda_nm is None:
            raise ValueError(f"{path}: coating lines need a lambda_nm line (the wavelengths of the index columns)")
        nl = ior.shape[0]
        thick = np.zeros(n, np.float32)
        index = np.zeros((nl, n), np.float32)
        for k, d, m in coats:
            if not 0 <= k < n or len(m) not in (1, nl) or thick[k] != 0:
                raise ValueError(f"{path}: bad coating line for interface {k}")
            thick[k] = d
            index[:, k] = m if len(m) == nl else m[0]
        lens["coatings"] = dict(lambda_nm=np.array(lambda_nm, np.float32), thickness_nm=thick, index=index)
    if layers:
        if lambda_nm is None:
            raise ValueError(f"{path}: layer lines need a lambda_nm line (the wavelengths of the index columns)")
        nl = ior.shape[0]
        n_layers = np.zeros(n, np.int32)
        thick = np.zeros((MAX_COAT_LAYERS, n), np.float32)
        index = np.zeros((MAX_COAT_LAYERS, nl, n), np.float32)
        coated = {k for k, _, _ in coats}
        for k, d, m in layers:
            if not 0 <= k < n or len(m) not in (1, nl):
                raise ValueError(f"{path}: bad layer line for interface {k}")
            if k in coated:
                raise ValueError(f"{path}: interface {k} has a coating line and layer lines")
            if n_layers[k] >= MAX_COAT_LAYERS:
                raise ValueError(f"{path}: more than {MAX_COAT_LAYERS} layers on interface {k}")
            thick[n_layers[k], k] = d
            index[n_layers[k], :, k] = m if len(m) == nl else m[0]
            n_layers[k] += 1
        if coats:                    # a film is a stack of one layer: everything goes through the stacks' setter
            c = lens.pop("coatings")
            for k in coated:
                n_layers[k], thick[0, k], index[0, :, k] = 1, c["thickness_nm"][k], c["index"][:, k]
        lens["coating_stacks"] = dict(lambda_nm=np.array(lambda_nm, np.float32), n_layers=n_layers, thickness_nm=thick,
                                      index=index)
    return lens


MAX_COAT_LAYERS = 6      # LF_MAX_COAT_LAYERS
MAX_ASPH_COEF = 6        # LF_MAX_ASPH_COEF
CULL_ASPHERIC = 9        # LF_CULL_ASPHERIC
ASPH_ALIVE, ASPH_MISSED, ASPH_APERTURE, ASPH_TIR = 0, 1, 2, 3   # the fates of lf_asphere_event
CULL_ANAMORPHIC = 10     # LF_CULL_ANAMORPHIC
CULL_POSED = 11          # LF_CULL_POSED
SENSOR_GHOSTS_OFF, SENSOR_GHOSTS_ADD, SENSOR_GHOSTS_ONLY = 0, 1, 2   # the modes of lf_set_sensor_ghosts
SENSOR_SURFACES_CENTRED, SENSOR_SURFACES_POSED = 0, 1                # lf_set_sensor_ghost_surfaces: may a sensor path meet posed interfaces


def sensor_path_sequence(n_surfaces, stop_index, i):
    """The events of the sensor path of interface i in marching order: interface | reflect << 8 | forward << 9, n_surfaces
    standing for the sensor's mirror (host arithmetic)."""
    out = np.zeros(3 * max(int(n_surfaces), 1), np.int32)
    n_ev = C.c_int()
    st = load_library().lf_sensor_path_sequence(int(n_surfaces), int(stop_index), int(i), _fp(out, C.c_int), len(out), C.byref(n_ev))
    if st != 0:
        raise LensFlareError(st, "lf_sensor_path_sequence")
    return out[:n_ev.value].copy()


def sensor_mirror_event(rays, dzv, half_width_mm, half_height_mm):
    """The sensor's event on n rays {x, y, z, Kx, Ky, Kz} (host arithmetic, the kernels' own definition): (out n x 6, inside n)."""
    lib = load_library()
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    out = np.zeros_like(rays)
    inside = np.zeros(len(rays), np.int32)
    one = C.c_int()
    for k in range(len(rays)):
        st = lib.lf_sensor_mirror_event(_fp(rays[k], C.c_float), C.c_float(dzv), C.c_float(half_width_mm), C.c_float(half_height_mm),
                                        _fp(out[k], C.c_float), C.byref(one))
        if st != 0:
            raise LensFlareError(st, "lf_sensor_mirror_event")
        inside[k] = one.value
    return out, inside


def biconic_sag(curvature_x, curvature_y, conic_x, conic_y, x, y):
    """(z, dz/dx, dz/dy) of a biconic surface at (x, y) in the march's float32 arithmetic (lf_biconic_sag, host only)."""
    z, zx, zy = C.c_float(), C.c_float(), C.c_float()
    st = load_library().lf_biconic_sag(C.c_float(curvature_x), C.c_float(curvature_y), C.c_float(conic_x), C.c_float(conic_y),
                                       C.c_float(x), C.c_float(y), C.byref(z), C.byref(zx), C.byref(zy))
    if st != 0:
        raise LensFlareError(st, "lf_biconic_sag")
    return z.value, zx.value, zy.value


def biconic_event(curvature_x, curvature_y, conic_x, conic_y, semi_aperture, n_in, n_out, reflect, forward, dzv, rays):
    """One event on a biconic interface for each of the n x 6 rays {x, y, z, Kx, Ky, Kz}, host arithmetic
    (lf_biconic_event): (out n x 8 = {ray, sq, ct}, fates n)."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    out = np.zeros((len(rays), 8), np.float32)
    fates = np.zeros(len(rays), np.int32)
    fn = load_library().lf_biconic_event
    ro = (C.c_float * 6)()
    sq, ct, fate = C.c_float(), C.c_float(), C.c_int()
    consts = (C.c_float(curvature_x), C.c_float(curvature_y), C.c_float(conic_x), C.c_float(conic_y), C.c_float(semi_aperture),
              C.c_float(n_in), C.c_float(n_out), int(bool(reflect)), int(bool(forward)), C.c_float(dzv))
    for i in range(len(rays)):
        st = fn(*consts, _fp(rays[i], C.c_float), ro, C.byref(sq), C.byref(ct), C.byref(fate))
        if st != 0:
            raise LensFlareError(st, "lf_biconic_event")
        out[i, :6] = ro[:]
        out[i, 6], out[i, 7], fates[i] = sq.value, ct.value, fate.value
    return out, fates


def pose_rotation(tilt_deg):
    """R = Rx(ax) Ry(ay) Rz(az) of lf_set_lens_poses (float64; angles right-handed, in degrees)."""
    ax, ay, az = np.deg2rad(np.asarray(tilt_deg, np.float64))
    ca, sa, cb, sb, cg, sg = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return rx @ ry @ rz


def pose_group(lens, first, last, pivot_z, decentre, tilt_deg):
    """The pose records of the rigid group of interfaces first .. last of `lens`, turned by tilt_deg about the point
    (0, 0, pivot_z) of the axis and then moved by decentre: the same R on every interface and
    t_k = d + (R - I) (0, 0, z_k - pivot_z), z_k the vertex of interface k measured from interface 0's (the sum of the
    thicknesses before it).  Returns dict(on, decentre n x 3, tilt_deg n x 3) for set_lens_poses; an interface outside the
    group keeps on = 0.  (This is how an ELEMENT is tilted: its faces need different records.)"""
    n = int(lens["n"])
    if not 0 <= first <= last < n:
        raise ValueError("pose_group: 0 <= first <= last < n")
    z = np.concatenate([[0.0], np.cumsum(np.asarray(lens["thickness"], np.float64)[:-1])])
    R = pose_rotation(tilt_deg)
    d = np.asarray(decentre, np.float64)
    on = np.zeros(n, np.int32)
    t = np.zeros((n, 3), np.float32)
    a = np.zeros((n, 3), np.float32)
    for k in range(first, last + 1):
        on[k] = 1
        t[k] = d + (R - np.eye(3)) @ np.array([0.0, 0.0, z[k] - pivot_z])
        a[k] = tilt_deg
    return dict(on=on, decentre=t, tilt_deg=a)


def _pose_event_consts(curvature_x, curvature_y, conic_x, conic_y, asphere, decentre, tilt_deg, semi_aperture, n_in, n_out,
                       reflect, forward, dzv):
    kappa, coef = (0.0, ()) if asphere is None else asphere
    a = np.ascontiguousarray(coef, np.float32).ravel()
    d = np.ascontiguousarray(decentre, np.float32).ravel()
    t = np.ascontiguousarray(tilt_deg, np.float32).ravel()
    if len(d) != 3 or len(t) != 3:
        raise ValueError("decentre and tilt_deg hold three values")
    keep = (a, d, t)
    return keep, (C.c_float(curvature_x), C.c_float(curvature_y), C.c_float(conic_x), C.c_float(conic_y), int(asphere is not None),
                  C.c_float(kappa), _fp(a, C.c_float) if len(a) else None, len(a), _fp(d, C.c_float), _fp(t, C.c_float),
                  C.c_float(semi_aperture), C.c_float(n_in), C.c_float(n_out), int(bool(reflect)), int(bool(forward)),
                  C.c_float(dzv))


def pose_event(curvature_x, curvature_y, conic_x, conic_y, asphere, decentre, tilt_deg, semi_aperture, n_in, n_out, reflect,
               forward, dzv, rays):
    """One event on a posed interface for each of the n x 6 rays {x, y, z, Kx, Ky, Kz}, host arithmetic (lf_pose_event):
    biconic_event's arguments, `asphere` = None or (kappa, coef) -- then the surface of revolution of curvature_y -- and the
    pose (decentre mm, tilt_deg).  (out n x 8 = {ray, sq, ct}, fates n)."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    out = np.zeros((len(rays), 8), np.float32)
    fates = np.zeros(len(rays), np.int32)
    fn = load_library().lf_pose_event
    ro = (C.c_float * 6)()
    sq, ct, fate = C.c_float(), C.c_float(), C.c_int()
    keep, consts = _pose_event_consts(curvature_x, curvature_y, conic_x, conic_y, asphere, decentre, tilt_deg, semi_aperture,
                                      n_in, n_out, reflect, forward, dzv)
    for i in range(len(rays)):
        st = fn(*consts, _fp(rays[i], C.c_float), ro, C.byref(sq), C.byref(ct), C.byref(fate))
        if st != 0:
            raise LensFlareError(st, "lf_pose_event")
        out[i, :6] = ro[:]
        out[i, 6], out[i, 7], fates[i] = sq.value, ct.value, fate.value
    return out, fates


def asphere_sag(curvature, conic, coef, r2):
    """(z, dz/dr2) of an aspheric surface at r2 = r^2 in the march's float32 arithmetic (lf_asphere_sag, host only)."""
    a = np.ascontiguousarray(coef, np.float32).ravel()
    z, zp = C.c_float(), C.c_float()
    st = load_library().lf_asphere_sag(C.c_float(curvature), C.c_float(conic), len(a), _fp(a, C.c_float), C.c_float(r2),
                                       C.byref(z), C.byref(zp))
    if st != 0:
        raise LensFlareError(st, "lf_asphere_sag")
    return z.value, zp.value


def asphere_event(curvature, conic, coef, semi_aperture, n_in, n_out, reflect, forward, dzv, rays):
    """One event on an aspheric interface for each of the n x 6 rays {x, y, z, Kx, Ky, Kz}, host arithmetic
    (lf_asphere_event): (out n x 8 = {ray, sq, ct}, fates n)."""
    a = np.ascontiguousarray(coef, np.float32).ravel()
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    out = np.zeros((len(rays), 8), np.float32)
    fates = np.zeros(len(rays), np.int32)
    fn = load_library().lf_asphere_event
    ro = (C.c_float * 6)()
    sq, ct, fate = C.c_float(), C.c_float(), C.c_int()
    consts = (C.c_float(curvature), C.c_float(conic), len(a), _fp(a, C.c_float), C.c_float(semi_aperture), C.c_float(n_in),
              C.c_float(n_out), int(bool(reflect)), int(bool(forward)), C.c_float(dzv))
    for i in range(len(rays)):
        st = fn(*consts, _fp(rays[i], C.c_float), ro, C.byref(sq), C.byref(ct), C.byref(fate))
        if st != 0:
            raise LensFlareError(st, "lf_asphere_event")
        out[i, :6] = ro[:]
        out[i, 6], out[i, 7], fates[i] = sq.value, ct.value, fate.value
    return out, fates


def coating_stack_reflectance(n_in, n_film, thickness_nm, n_out, lambda_nm, cos_in):
    """(R_s, R_p, R) of one interface under a stack of layers in the march's float32 arithmetic
    (lf_coating_stack_reflectance, host only): n_film[i], thickness_nm[i] in the order the ray meets them."""
    m = np.ascontiguousarray(n_film, np.float32).ravel()
    d = np.ascontiguousarray(thickness_nm, np.float32).ravel()
    if len(m) != len(d):
        raise ValueError("one index and one thickness per layer")
    out = (C.c_float * 3)()
    st = load_library().lf_coating_stack_reflectance(C.c_float(n_in), len(m), _fp(m, C.c_float), _fp(d, C.c_float),
                                                     C.c_float(n_out), C.c_float(lambda_nm), C.c_float(cos_in), out)
    if st != 0:
        raise LensFlareError(st, "lf_coating_stack_reflectance")
    return float(out[0]), float(out[1]), float(out[2])


def quarter_wave_thickness(m, lambda_nm):
    """Physical thickness (nm) of a quarter-wave film of index m at wavelength lambda_nm: lambda / (4 m)."""
    return float(lambda_nm) / (4.0 * float(m))


def coating_reflectance(n_in, n_film, n_out, thickness_nm, lambda_nm, cos_in):
    """(R_s, R_p, R) of one coated interface in the march's float32 arithmetic (lf_coating_reflectance, host only):
    a ray arriving in n_in at incidence cosine cos_in; thickness 0 = the bare interface."""
    out = (C.c_float * 3)()
    st = load_library().lf_coating_reflectance(C.c_float(n_in), C.c_float(n_film), C.c_float(n_out),
                                               C.c_float(thickness_nm), C.c_float(lambda_nm), C.c_float(cos_in), out)
    if st != 0:
        raise LensFlareError(st, "lf_coating_reflectance")
    return float(out[0]), float(out[1]), float(out[2])


# the kinds of lf_set_lights_ex: a direction, or a position in lens millimetres (front vertex at z = 0, the scene at z < 0)
LIGHT_DIRECTIONAL, LIGHT_POINT = 0, 1


def validate_light(kind, vec, radiance, angular_radius, front_radius, front_semi_aperture):
    """(status, message) of one light as lf_set_lights_ex validates it against a front element of the given radius
    (0: flat) and semi-aperture (lf_validate_light, host only): status 0 = accepted."""
    v = np.ascontiguousarray(vec, np.float32).reshape(3)
    r = np.ascontiguousarray(radiance, np.float32).reshape(3)
    msg = C.create_string_buffer(512)
    st = load_library().lf_validate_light(int(kind), _fp(v, C.c_float), _fp(r, C.c_float), C.c_float(angular_radius),
                                          C.c_float(front_radius), C.c_float(front_semi_aperture), msg, C.c_size_t(512))
    return int(st), msg.value.decode()


def light_lobe_factor(kind, vec, angular_radius, ray):
    """(q, inside) of one exit ray {origin xyz in lens mm (z absolute), direction xyz} for one light in the march's float32
    arithmetic (lf_light_lobe_factor, host only): a point light's is the definition the kernels call."""
    v = np.ascontiguousarray(vec, np.float32).reshape(3)
    r = np.ascontiguousarray(ray, np.float32).reshape(6)
    q, inside = C.c_float(), C.c_int()
    st = load_library().lf_light_lobe_factor(int(kind), _fp(v, C.c_float), C.c_float(angular_radius), _fp(r, C.c_float),
                                             C.byref(q), C.byref(inside))
    if st != 0:
        raise LensFlareError(st, "lf_light_lobe_factor")
    return float(q.value), int(inside.value)


def light_lobe_factors(kind, vec, angular_radius, rays):
    """light_lobe_factor over n x 6 rays -> (q float32 array, inside bool array)"""
    lib = load_library()
    v = np.ascontiguousarray(vec, np.float32).reshape(3)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    qs, ins = np.zeros(len(r), np.float32), np.zeros(len(r), bool)
    q, inside = C.c_float(), C.c_int()
    fn, vp, ar, base = lib.lf_light_lobe_factor, _fp(v, C.c_float), C.c_float(angular_radius), r.ctypes.data
    for i in range(len(r)):
        st = fn(int(kind), vp, ar, C.cast(base + 24 * i, C.POINTER(C.c_float)), C.byref(q), C.byref(inside))
        if st != 0:
            raise LensFlareError(st, "lf_light_lobe_factor")
        qs[i], ins[i] = q.value, bool(inside.value)
    return qs, ins


# where the shadow ray of a point light ends under ghost occlusion (lf_set_ghost_occlusion_reach): at the sky (the default: occlusion
# with a point light installed is refused) or at the light
OCCLUSION_REACH_SKY, OCCLUSION_REACH_LIGHT = 0, 1
# which interfaces the lens camera's primary path may meet (lf_set_lens_camera_surfaces): spheres, flats and the stop (the default: a
# lens with aspheric or biconic records is refused, as it always was), every recorded kind, or those and posed interfaces
# (lf_set_lens_poses).  Bits: 1 records, 2 poses; 2 alone is no setting
LENSCAM_SURFACES_SPHERICAL, LENSCAM_SURFACES_ALL, LENSCAM_SURFACES_POSED = 0, 1, 3


def ghost_shadow_reach(kind, vec, rays, world_per_mm):
    """reach_k of n x 6 exit rays {origin xyz in lens mm (z absolute), direction xyz} for one light, float64 array of n: +inf for
    LIGHT_DIRECTIONAL; for LIGHT_POINT at vec the ray parameter, in world units, of the ray's point nearest the lamp, never
    below 0 (lf_ghost_shadow_reach, host only: the definition the occlusion kernels call)."""
    if int(kind) not in (LIGHT_DIRECTIONAL, LIGHT_POINT):
        raise ValueError("ghost_shadow_reach: kind must be LIGHT_DIRECTIONAL or LIGHT_POINT")
    v = np.asarray(vec)
    if v.shape != (3,):
        raise ValueError("ghost_shadow_reach: vec must be 3 numbers")
    r = np.asarray(rays)
    if r.ndim != 2 or r.shape[1] != 6:
        raise ValueError("ghost_shadow_reach: rays must be n x 6 (origin xyz in lens mm, direction xyz)")
    v, r, w = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(r, np.float32), float(world_per_mm)
    if not np.isfinite(v).all() or not np.isfinite(r).all() or not (np.abs(r[:, 3:]).max(axis=1) > 0.0).all():
        raise ValueError("ghost_shadow_reach: vec and rays must be finite, directions non-zero")
    if not (w > 0.0 and np.isfinite(w)):
        raise ValueError("ghost_shadow_reach: world_per_mm must be > 0 and finite")
    out, t = np.zeros(len(r), np.float64), C.c_double()
    fn, vp, base = load_library().lf_ghost_shadow_reach, _fp(v, C.c_float), r.ctypes.data
    for i in range(len(r)):
        st = fn(int(kind), vp, C.cast(base + 24 * i, C.POINTER(C.c_float)), C.c_double(w), C.byref(t))
        if st != 0:
            raise LensFlareError(st, "lf_ghost_shadow_reach")
        out[i] = t.value
    return out


# where the shadow rays of flare occlusion start (lf_set_flare_occlusion): at the camera position, or on the front element's
# vertex plane in lens millimetres (needs a lens and the scale world_per_mm)
FLARE_ORIGIN_CAMERA, FLARE_ORIGIN_FRONT_ELEMENT = 0, 1
MAX_FLARES = 8   # LF_MAX_FLARES


def _flare_occlusion_args(who, rays_per_light, angular_radius, origin, world_per_mm=None):
    """the setter's validation, before anything reaches the library"""
    R = rays_per_light
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 64 <= int(R) <= 4096 or int(R) % 64:
        raise ValueError(f"{who}: rays_per_light must be a multiple of 64 in [64, 4096]")
    a = float(angular_radius)
    if not (np.isfinite(a) and 0.0 <= a <= 0.5):
        raise ValueError(f"{who}: angular_radius must be finite and in [0, 0.5]")
    if isinstance(origin, bool) or not isinstance(origin, (int, np.integer)) or int(origin) not in (FLARE_ORIGIN_CAMERA, FLARE_ORIGIN_FRONT_ELEMENT):
        raise ValueError(f"{who}: origin must be FLARE_ORIGIN_CAMERA (0) or FLARE_ORIGIN_FRONT_ELEMENT (1)")
    if world_per_mm is not None and int(origin) == FLARE_ORIGIN_FRONT_ELEMENT:
        w = float(world_per_mm)
        if not (w > 0.0 and np.isfinite(w)):
            raise ValueError(f"{who}: world_per_mm must be > 0 and finite under FLARE_ORIGIN_FRONT_ELEMENT")
    return int(R), a, int(origin)


def flare_shadow_samples(rays_per_light):
    """R x 4 float32 (a, b, c, d): the point of the unit aperture disc and of the light's unit disc of each shadow ray
    (lf_flare_shadow_samples, host only: the definition of the resident table)"""
    R, _, _ = _flare_occlusion_args("flare_shadow_samples", rays_per_light, 0.0, FLARE_ORIGIN_CAMERA)
    out = np.zeros((R, 4), np.float32)
    st = load_library().lf_flare_shadow_samples(R, _fp(out, C.c_float))
    if st != 0:
        raise LensFlareError(st, "lf_flare_shadow_samples")
    return out


def flare_shadow_rays(rays_per_light, flare_origin, hfov_deg, vfov_deg, angular_radius, origin, front_semi_aperture=0.0):
    """R x 6 float32 {origin xyz in lens mm, direction xyz}: the shadow rays of the flare stored at screen position
    flare_origin (lf_flare_shadow_rays, host only: the definition the visibility kernel reproduces bit for bit)"""
    R, a, origin = _flare_occlusion_args("flare_shadow_rays", rays_per_light, angular_radius, origin)
    o = np.ascontiguousarray(flare_origin, np.float64).reshape(2)
    if not np.isfinite(o).all() or not (0.0 < float(hfov_deg) < 180.0 and 0.0 < float(vfov_deg) < 180.0):
        raise ValueError("flare_shadow_rays: the flare origin must be finite, the fields of view inside (0, 180)")
    h0 = float(front_semi_aperture)
    if origin == FLARE_ORIGIN_FRONT_ELEMENT and not (h0 > 0.0 and np.isfinite(h0)):
        raise ValueError("flare_shadow_rays: front_semi_aperture must be > 0 under FLARE_ORIGIN_FRONT_ELEMENT")
    out = np.zeros((R, 6), np.float32)
    st = load_library().lf_flare_shadow_rays(R, _fp(o, C.c_double), C.c_double(float(hfov_deg)), C.c_double(float(vfov_deg)),
                                             C.c_float(a), origin, C.c_float(h0), _fp(out, C.c_float))
    if st != 0:
        raise LensFlareError(st, "lf_flare_shadow_rays")
    return out


# the third kind, known to the twelve-float calls alone (lf_set_lights_geom): a one-sided rectangle -- centre, direction,
# dim_x, dim_y (full edge vectors) in lens millimetres
LIGHT_AREA, LIGHT_GEOM_FLOATS = 2, 12


def _geom(geom):
    g = np.ascontiguousarray(geom, np.float32).reshape(-1)
    if len(g) == 3:
        g = np.concatenate([g, np.zeros(9, np.float32)])
    if len(g) != LIGHT_GEOM_FLOATS:
        raise ValueError("a light's geometry is 12 floats (kinds 0 and 1: the first 3 count)")
    return np.ascontiguousarray(g, np.float32)


def validate_light_geom(kind, geom, radiance, angular_radius, front_radius, front_semi_aperture):
    """(status, message) of one light as lf_set_lights_geom validates it (lf_validate_light_geom, host only)"""
    g = _geom(geom)
    r = np.ascontiguousarray(radiance, np.float32).reshape(3)
    msg = C.create_string_buffer(512)
    st = load_library().lf_validate_light_geom(int(kind), _fp(g, C.c_float), _fp(r, C.c_float), C.c_float(angular_radius),
                                               C.c_float(front_radius), C.c_float(front_semi_aperture), msg, C.c_size_t(512))
    return int(st), msg.value.decode()


def light_geom_factors(kind, geom, angular_radius, rays):
    """n x 6 exit rays, one light -> (factor float32, inside bool, t float64) (lf_light_geom_factor, host only: an area light's
    is the definition the kernels call; t = the ray parameter of its plane)"""
    g = _geom(geom)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    fs, ins, ts = np.zeros(len(r), np.float32), np.zeros(len(r), bool), np.zeros(len(r), np.float64)
    f, inside, t = C.c_float(), C.c_int(), C.c_double()
    fn, gp, ar, base = load_library().lf_light_geom_factor, _fp(g, C.c_float), C.c_float(angular_radius), r.ctypes.data
    for i in range(len(r)):
        st = fn(int(kind), gp, ar, C.cast(base + 24 * i, C.POINTER(C.c_float)), C.byref(f), C.byref(inside), C.byref(t))
        if st != 0:
            raise LensFlareError(st, "lf_light_geom_factor")
        fs[i], ins[i], ts[i] = f.value, bool(inside.value), t.value
    return fs, ins, ts


def area_light_pretest(geom, rays):
    """does the pre-test of an area light admit each of n x 6 exit rays (lf_area_light_pretest, host only) -> bool array"""
    g = _geom(geom)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    out, a = np.zeros(len(r), bool), C.c_int()
    fn, gp, base = load_library().lf_area_light_pretest, _fp(g, C.c_float), r.ctypes.data
    for i in range(len(r)):
        st = fn(gp, C.cast(base + 24 * i, C.POINTER(C.c_float)), C.byref(a))
        if st != 0:
            raise LensFlareError(st, "lf_area_light_pretest")
        out[i] = bool(a.value)
    return out


def ghost_shadow_reach_geom(kind, geom, rays, world_per_mm):
    """reach of n x 6 exit rays for one light of any kind, float64 array (lf_ghost_shadow_reach_geom, host only): an area
    light's shadow ray ends EPS_F before its rectangle's plane"""
    g = _geom(geom)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    out, t = np.zeros(len(r), np.float64), C.c_double()
    fn, gp, base = load_library().lf_ghost_shadow_reach_geom, _fp(g, C.c_float), r.ctypes.data
    for i in range(len(r)):
        st = fn(int(kind), gp, C.cast(base + 24 * i, C.POINTER(C.c_float)), C.c_double(float(world_per_mm)), C.byref(t))
        if st != 0:
            raise LensFlareError(st, "lf_ghost_shadow_reach_geom")
        out[i] = t.value
    return out


def area_light_cull_cone(geom, front_radius, front_semi_aperture):
    """(dir float32 x 3, rho) the cull table takes an area light as (lf_area_light_cull_cone, host only)"""
    g = _geom(geom)
    d, rho = np.zeros(3, np.float32), C.c_float()
    st = load_library().lf_area_light_cull_cone(_fp(g, C.c_float), C.c_float(front_radius), C.c_float(front_semi_aperture),
                                                _fp(d, C.c_float), C.byref(rho))
    if st != 0:
        raise LensFlareError(st, "lf_area_light_cull_cone")
    return d, float(rho.value)


# how the march and the lens camera read the stop mask (lf_set_mask_filter)
MASK_NEAREST, MASK_BILINEAR = 0, 1


def mask_lookup(texels, u, v, filter=MASK_BILINEAR):
    """(value, open) of the stop-mask lookup in the march's float32 arithmetic (lf_mask_lookup, host only) at the
    stop-plane point (u, v) = (hx, hy) / stop_h: the transmission multiplied into the weight, and whether the ray
    survives the mask."""
    t = np.ascontiguousarray(texels, np.float32)
    h, w = t.shape
    value, alive = C.c_float(), C.c_int()
    st = load_library().lf_mask_lookup(_fp(t, C.c_float), w, h, int(filter), C.c_float(u), C.c_float(v),
                                       C.byref(value), C.byref(alive))
    if st != 0:
        raise LensFlareError(st, "lf_mask_lookup")
    return float(value.value), int(alive.value)


# Fraunhofer lines of the three index columns of the shipped prescriptions (C, d, F)
LINES_NM = (656.3, 587.6, 486.1)


def cauchy_indices(lens3, lambda_nm):
    """"indices by a 2-term Cauchy fit through each glass's three tabulated values"
    (the reference tabulates three per glass, pathtracer.cpp:553-555): n(lambda) = A + B / lambda^2, A and
    B by least squares through (C, d, F) of every interface; air and the stop stay exactly 1."""
    lam = np.asarray(lambda_nm, np.float64)
    basis = np.stack([np.ones(3), 1.0 / np.square(np.array(LINES_NM))], axis=1)   # 3 x 2
    ior3 = np.asarray(lens3["ior"], np.float64)                                 # 3 x n
    coef, *_ = np.linalg.lstsq(basis, ior3, rcond=None)                         # 2 x n
    out = coef[0][None, :] + coef[1][None, :] / np.square(lam)[:, None]
    out[:, np.all(ior3 == 1.0, axis=0)] = 1.0
    return out.astype(np.float32)


def spectral_weights(lambda_nm):
    """RGB weight of every wavelength (tents centred on the C, d, F lines, normalised so that the
    weights of a channel sum to 1) and the starburst's scale lambda_d / lambda (its pattern grows
    with the wavelength)."""
    lam = np.asarray(lambda_nm, np.float64)
    t = np.interp(-lam, [-LINES_NM[0], -LINES_NM[1], -LINES_NM[2]], [0.0, 1.0, 2.0])
    w = np.maximum(0.0, 1.0 - np.abs(t[:, None] - np.arange(3)[None, :]))
    tot = w.sum(axis=0, keepdims=True)
    w = np.where(tot > 0, w / np.where(tot > 0, tot, 1.0), 0.0)   # (a channel no wavelength reaches stays dark)
    return w.astype(np.float32), LINES_NM[1] / lam


def spectral_lens(lens3, n_lambda=8):
    """The prescription with n_lambda index columns by the Cauchy fit, wavelengths equally spaced from the
    C to the F line -> (lens, rgb weights, starburst scales).  data/dgauss11_8lambda.lens is
    spectral_lens(dgauss11.lens, 8) written out (data/make_spectral_lens.py; tests/test_spectral_lens_cpu.py)."""
    lam = np.linspace(LINES_NM[0], LINES_NM[2], n_lambda) if n_lambda > 1 else np.array([LINES_NM[1]])
    lens = dict(lens3, ior=cauchy_indices(lens3, lam), lambda_nm=lam)
    w, scale = spectral_weights(lam)
    return lens, w, scale


def paraxial_efl(lens, lam=None):
    """Paraxial focal length of a prescription dict (host arithmetic, needs no device)."""
    lib = load_library()
    ior = np.ascontiguousarray(lens["ior"], np.float32)
    lam = ior.shape[0] // 2 if lam is None else lam
    r = np.ascontiguousarray(lens["radius"], np.float32)
    t = np.ascontiguousarray(lens["thickness"], np.float32)
    row = np.ascontiguousarray(ior[lam], np.float32)
    out = C.c_double()
    st = lib.lf_paraxial_efl(int(lens["n"]), int(lens["stop"]), _fp(r, C.c_float), _fp(t, C.c_float),
                             _fp(row, C.c_float), C.byref(out))
    if st != 0:
        raise LensFlareError(st, "lf_paraxial_efl")
    return out.value


def paraxial_image_scale(lens, lam=None):
    """lf_paraxial_image_scale: chief-ray landing height per unit field angle on the sensor as the
    prescription dict places it (what lf_set_sun_from_flares(efl_mm <= 0) uses; host arithmetic)."""
    lib = load_library()
    ior = np.ascontiguousarray(lens["ior"], np.float32)
    lam = ior.shape[0] // 2 if lam is None else lam
    r = np.ascontiguousarray(lens["radius"], np.float32)
    t = np.ascontiguousarray(lens["thickness"], np.float32)
    row = np.ascontiguousarray(ior[lam], np.float32)
    out = C.c_double()
    st = lib.lf_paraxial_image_scale(int(lens["n"]), int(lens["stop"]), _fp(r, C.c_float), _fp(t, C.c_float),
                                     _fp(row, C.c_float), C.byref(out))
    if st != 0:
        raise LensFlareError(st, "lf_paraxial_image_scale")
    return out.value


def collada_check(path):
    """lf_collada_check: None if the device scene term can render the file, else the reason (no device needed)."""
    msg = C.create_string_buffer(512)
    st = load_library().lf_collada_check(os.fsencode(path), msg, C.c_size_t(512))
    return None if st == 0 else msg.value.decode()


def aim_camera(pos, world_point, ns, hfov_deg, vfov_deg):
    """Row-major c2w of a camera at `pos` under which `world_point` projects to the normalised screen
    position `ns` (Camera::analyze_world_coord, camera.cpp:245-273): any rotation that maps the
    camera-space direction of that screen point onto the direction towards the point."""
    import math
    ex, ey = math.tan(math.radians(hfov_deg) / 2), math.tan(math.radians(vfov_deg) / 2)
    d_cam = np.array([(2 * ns[0] - 1) * ex, (2 * ns[1] - 1) * ey, -1.0])
    d_cam /= np.linalg.norm(d_cam)
    fwd = np.asarray(world_point, float) - np.asarray(pos, float)
    fwd /= np.linalg.norm(fwd)

    def frame(z):
        h = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
        x = np.cross(h, z); x /= np.linalg.norm(x)
        return np.column_stack([x, np.cross(z, x), z])
    return frame(fwd) @ frame(d_cam).T


COMM_ID_BYTES = 128


def comm_available():
    """lf_comm_available: can RCCL be loaded in this process? (no blocking call, no device)"""
    return load_library().lf_comm_available() == 0


def comm_unique_id():
    """lf_comm_get_unique_id: the RCCL id rank 0 makes and the host shares (bytes)."""
    buf = (C.c_ubyte * COMM_ID_BYTES)()
    st = load_library().lf_comm_get_unique_id(buf)
    if st != 0:
        raise LensFlareError(st, "lf_comm_get_unique_id (is librccl.so.1 installed?)")
    return bytes(buf)


class LensFlare:
    """One context = one GPU.  Thin, checked wrappers; names follow include/lensflare.h."""

    def __init__(self, device=0, _borrowed=None):
        self.lib = load_library()
        self.lib.lf_group_ctx.restype = C.c_void_p
        self.W = self.H = 0
        self._owned = _borrowed is None
        if _borrowed is not None:
            self.ctx = C.c_void_p(_borrowed)
            return
        self.ctx = C.c_void_p()
        st = self.lib.lf_create(C.byref(self.ctx), int(device))
        if st != 0:
            self.ctx = C.c_void_p()
            raise LensFlareError(st, "lf_create failed (no gfx950 device visible?)")

    def close(self):
        if self.ctx and self._owned:
            # (LF_ERR_STATE: a communicator call this host gave up on -- comm_poison -- is still blocked in another
            # thread and stands on the context: the library leaks it on purpose rather than free it under that thread)
            self.leaked = self.lib.lf_destroy(self.ctx) != 0
        self.ctx = C.c_void_p()

    def comm_poison(self):
        """Give up on a communicator call that is blocked in another thread (sharding.call_with_deadline's on_expire):
        whatever that call still does, it publishes nothing into this context any more; every later comm_* call is
        refused; close() leaks the context while the call has not come back."""
        self.lib.lf_comm_poison(self.ctx)

    def comm_is_poisoned(self):
        return bool(self.lib.lf_comm_is_poisoned(self.ctx))

    # ---- multi-GPU, one process per GPU
    def comm_init_rank(self, nranks, rank, unique_id):
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._ck(self.lib.lf_comm_init_rank(self.ctx, int(nranks), int(rank), buf))

    def comm_gather(self, which):
        self._ck(self.lib.lf_comm_gather(self.ctx, int(which)))

    def comm_gather_async(self, which):
        """The exchange on the context's second stream: overlaps whatever is queued next."""
        self._ck(self.lib.lf_comm_gather_async(self.ctx, int(which)))

    def comm_wait(self):
        self._ck(self.lib.lf_comm_wait(self.ctx))

    def comm_info(self):
        """(nranks, rank) as RCCL reports them; (0, -1) without a communicator."""
        n, r = C.c_int(), C.c_int()
        self._ck(self.lib.lf_comm_info(self.ctx, C.byref(n), C.byref(r)))
        return n.value, r.value

    def comm_test(self):
        d = C.c_int()
        self._ck(self.lib.lf_comm_test(self.ctx, C.byref(d)))
        return bool(d.value)

    def comm_abort(self):
        self._ck(self.lib.lf_comm_abort(self.ctx))

    def comm_set_exchange_precision(self, bits):
        self._ck(self.lib.lf_comm_set_exchange_precision(self.ctx, int(bits)))

    def comm_exchange_plan(self, world):
        v = (C.c_uint64 * 6)()
        self._ck(self.lib.lf_comm_exchange_plan(self.ctx, int(world), v))
        return dict(sendcount=int(v[0]), element_bytes=int(v[1]), recv_offset_bytes=int(v[2]),
                    staging_bytes=int(v[3]), groups=int(v[4]), tile_row_elements=int(v[5]))

    def comm_destroy(self):
        self._ck(self.lib.lf_comm_destroy(self.ctx))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st):
        if st != 0:
            raise LensFlareError(st, self.lib.lf_last_error(self.ctx).decode())

    # ---- frame / params
    def set_stream(self, stream_ptr):
        self._ck(self.lib.lf_set_stream(self.ctx, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._ck(self.lib.lf_synchronize(self.ctx))

    def set_frame(self, W, H):
        self._ck(self.lib.lf_set_frame(self.ctx, int(W), int(H)))
        self.W, self.H = int(W), int(H)

    def set_band(self, y0, y1):
        self._ck(self.lib.lf_set_band(self.ctx, int(y0), int(y1)))

    def set_row_interleave(self, phase, period):
        self._ck(self.lib.lf_set_row_interleave(self.ctx, int(phase), int(period)))

    def set_block_deal(self, rank, nranks):
        """the frame dealt by 64 x 64-pixel blocks: block b (row-major) belongs to rank b % nranks (lf_set_block_deal)"""
        self._ck(self.lib.lf_set_block_deal(self.ctx, int(rank), int(nranks)))

    def set_params(self, ns_aa=1, flare_radius=25.0, flare_intensity=1.0):
        self._ck(self.lib.lf_set_params(self.ctx, int(ns_aa), C.c_double(flare_radius),
                                        C.c_double(flare_intensity)))
        self._ns_aa = int(ns_aa)

    # ---- inputs
    def set_aperture(self, slot, texels):
        texels = np.ascontiguousarray(texels, np.float32)
        h, w = texels.shape
        self._ck(self.lib.lf_set_aperture(self.ctx, int(slot), _fp(texels, C.c_float), w, h))

    def set_mask_filter(self, filter):
        """MASK_NEAREST (default) or MASK_BILINEAR: how the march and the lens camera read the stop mask."""
        self._ck(self.lib.lf_set_mask_filter(self.ctx, int(filter)))

    def mask_filter(self):
        f = C.c_int()
        self._ck(self.lib.lf_get_mask_filter(self.ctx, C.byref(f)))
        return f.value

    def aperture_stats(self, slot):
        st = ApertureStats()
        self._ck(self.lib.lf_get_aperture_stats(self.ctx, int(slot), C.byref(st)))
        return st

    def set_paraxial_lens(self, n=None, stop=None, thickness=None, curvature=None, ior_rgb=None):
        if thickness is None:
            self._ck(self.lib.lf_set_paraxial_lens(self.ctx, 0, 0, None, None, None))
            return
        th = np.ascontiguousarray(thickness, np.float32)
        cu = np.ascontiguousarray(curvature, np.float32)
        io = np.ascontiguousarray(ior_rgb, np.float32)
        self._ck(self.lib.lf_set_paraxial_lens(self.ctx, int(n), int(stop), _fp(th, C.c_float),
                                               _fp(cu, C.c_float), _fp(io, C.c_float)))

    def set_camera(self, c2w, pos, hfov_deg, vfov_deg):
        c2w = np.ascontiguousarray(c2w, np.float64).reshape(9)
        pos = np.ascontiguousarray(pos, np.float64).reshape(3)
        self._ck(self.lib.lf_set_camera(self.ctx, _fp(c2w, C.c_double), _fp(pos, C.c_double),
                                        C.c_double(hfov_deg), C.c_double(vfov_deg)))

    def find_sun_pos(self, lights):
        lights = np.ascontiguousarray(lights, np.float64).reshape(-1, 6)
        self._ck(self.lib.lf_find_sun_pos(self.ctx, _fp(lights, C.c_double), len(lights)))

    def set_flares(self, origins, radiance, axis_ray, angle_to_sun):
        o = np.ascontiguousarray(origins, np.float64).reshape(-1, 2)
        r = np.ascontiguousarray(radiance, np.float64).reshape(-1, 3)
        a = np.ascontiguousarray(axis_ray, np.float64).reshape(2)
        self._ck(self.lib.lf_set_flares(self.ctx, len(o), _fp(o, C.c_double), _fp(r, C.c_double),
                                        _fp(a, C.c_double), C.c_float(angle_to_sun)))

    def get_flares(self):
        n = C.c_int()
        o = np.zeros((8, 2), np.float64)
        r = np.zeros((8, 3), np.float64)
        a = np.zeros(2, np.float64)
        ang = C.c_float()
        self._ck(self.lib.lf_get_flares(self.ctx, C.byref(n), _fp(o, C.c_double), _fp(r, C.c_double),
                                        _fp(a, C.c_double), C.byref(ang)))
        return dict(n=n.value, origins=o[:n.value], radiance=r[:n.value], axis_ray=a,
                    angle_to_sun=ang.value)

    def set_jitter_mt19937(self, seed=5489, order=None):
        if order is None:
            self._ck(self.lib.lf_set_jitter_mt19937(self.ctx, C.c_uint32(seed), None, C.c_size_t(0)))
        else:
            order = np.ascontiguousarray(order, np.uint32)
            self._ck(self.lib.lf_set_jitter_mt19937(self.ctx, C.c_uint32(seed),
                                                    _fp(order, C.c_uint32), C.c_size_t(len(order))))

    def set_jitter_counter(self, key):
        self._ck(self.lib.lf_set_jitter_counter(self.ctx, C.c_uint64(key)))

    def set_scene_term(self, rgb):
        if rgb is None:
            self._ck(self.lib.lf_set_scene_term(self.ctx, None))
        else:
            rgb = np.ascontiguousarray(rgb, np.float64)
            assert rgb.size == self.W * self.H * 3
            self._ck(self.lib.lf_set_scene_term(self.ctx, _fp(rgb, C.c_double)))

    # ---- scene term
    def set_scene(self, spheres=(), tris=(), lights=()):
        """spheres: (cx,cy,cz,r,kind,a,b,c); tris: 18 numbers + (kind,a,b,c), kind 'd'|'e';
        lights: (type, x,y,z, r,g,b) with type 0 = directional (dirToLight), 1 = point."""
        mats, sp, spm, tp, tn, tm = [], [], [], [], [], []

        def mat(kind, a, b, c):
            # 'd' diffuse reflectance, 'e' emitted radiance, 'm' one of the reference's stub BSDFs
            # (mirror / glass / ...: f() = 0, a black occluder under its integrator)
            mats.append([1.0, a, b, c] if kind == "e" else [0.0, 0.0, 0.0, 0.0] if kind == "m" else [0.0, a, b, c])
            return len(mats) - 1

        for s in spheres:
            sp.append(list(s[:4])); spm.append(mat(*s[4:8]))
        for t in tris:
            tp.append(list(t[:9])); tn.append(list(t[9:18])); tm.append(mat(*t[18:22]))
        arr = lambda a, t: np.ascontiguousarray(np.array(a, t).reshape(-1))  # noqa: E731
        spa, spma = arr(sp, np.float64), arr(spm, np.int32)
        tpa, tna, tma = arr(tp, np.float64), arr(tn, np.float64), arr(tm, np.int32)
        ma, la = arr(mats, np.float64), arr(lights, np.float64)
        self._ck(self.lib.lf_set_scene(self.ctx, len(sp), _fp(spa, C.c_double), _fp(spma, C.c_int),
                                       len(tp), _fp(tpa, C.c_double), _fp(tna, C.c_double),
                                       _fp(tma, C.c_int), len(mats), _fp(ma, C.c_double),
                                       len(lights), _fp(la, C.c_double)))

    def set_scene_lights(self, rows):
        """rows: n x 16 {type, rgb, v0, v1, v2, v3} (include/lensflare.h, lf_set_scene_lights)."""
        r = np.ascontiguousarray(rows, np.float64).reshape(-1, 16)
        self._ck(self.lib.lf_set_scene_lights(self.ctx, len(r), _fp(r, C.c_double)))

    def set_light_samples(self, ns_area_light):
        self._ck(self.lib.lf_set_light_samples(self.ctx, int(ns_area_light)))

    def set_environment_map(self, rgb):
        """PathTracer::envLight: rgb = (h, w, 3) doubles (HDRImageBuffer::data), or None to remove it."""
        if rgb is None:
            self._ck(self.lib.lf_set_environment_map(self.ctx, 0, 0, None))
            return
        a = np.ascontiguousarray(rgb, np.float64)
        assert a.ndim == 3 and a.shape[2] == 3
        self._ck(self.lib.lf_set_environment_map(self.ctx, a.shape[1], a.shape[0], _fp(a, C.c_double)))

    def set_direct_hemisphere_sample(self, on):
        self._ck(self.lib.lf_set_direct_hemisphere_sample(self.ctx, 1 if on else 0))

    def load_collada(self, path, max_suns=8):
        """Row f3: parse a .dae, upload its static scene; returns (camera dict or None, sun lights
        as [[px, py, pz, r, g, b], ...] for find_sun_pos)."""
        cam = ColladaCamera()
        suns = np.zeros((max_suns, 6), np.float64)
        n = C.c_int(0)
        self._ck(self.lib.lf_load_collada(self.ctx, os.fsencode(path), C.byref(cam), _fp(suns, C.c_double),
                                          max_suns, C.byref(n)))
        camera = None
        if cam.present:
            camera = dict(hfov=cam.hfov, vfov=cam.vfov, nclip=cam.nclip, fclip=cam.fclip,
                          pos=list(cam.pos), dir=list(cam.dir), up=list(cam.up))
        return camera, suns[:min(n.value, max_suns)].tolist()

    def scene_bounds(self):
        lo, hi, n = (C.c_double * 3)(), (C.c_double * 3)(), C.c_int()
        self._ck(self.lib.lf_scene_bounds(self.ctx, lo, hi, C.byref(n)))
        return np.array(lo[:]), np.array(hi[:]), n.value

    def set_sampling(self, samples_per_batch=32, max_tolerance=0.05, n_clip=0.01, f_clip=100.0):
        self._ck(self.lib.lf_set_sampling(self.ctx, int(samples_per_batch), C.c_double(max_tolerance),
                                          C.c_double(n_clip), C.c_double(f_clip)))

    def render_scene_term(self):
        self._ck(self.lib.lf_render_scene_term(self.ctx))

    # ---- render
    def generate_ghost_buffer(self):
        self._ck(self.lib.lf_generate_ghost_buffer(self.ctx))

    def render_flare_layer(self):
        self._ck(self.lib.lf_render_flare_layer(self.ctx))

    # ---- read back
    def read_tile(self, which, x0, y0, x1, y1, pixel_stride=3):
        out = np.zeros((y1 - y0, x1 - x0, pixel_stride), np.float64)
        self._ck(self.lib.lf_read_tile(self.ctx, int(which), x0, y0, x1, y1, _fp(out, C.c_double),
                                       C.c_size_t(pixel_stride)))
        return out

    def read_buffer(self, which):
        return self.read_tile(which, 0, 0, self.W, self.H)

    def read_pixel(self, which, x, y):
        rgb = (C.c_double * 3)()
        self._ck(self.lib.lf_read_pixel(self.ctx, int(which), int(x), int(y), rgb))
        return np.array(rgb[:])

    def write_to_framebuffer(self, x0, y0, x1, y1):
        out = np.zeros((y1 - y0, x1 - x0), np.uint32)
        self._ck(self.lib.lf_write_to_framebuffer(self.ctx, x0, y0, x1, y1, _fp(out, C.c_uint32),
                                                  C.c_size_t(x1 - x0)))
        return out

    def save_image_rgba(self):
        out = np.zeros((self.H, self.W), np.uint32)
        self._ck(self.lib.lf_save_image_rgba(self.ctx, _fp(out, C.c_uint32)))
        return out

    def device_buffer(self, which):
        p = C.c_void_p()
        n = C.c_size_t()
        self._ck(self.lib.lf_device_buffer(self.ctx, int(which), C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- geometric lens
    def set_lens(self, lens):
        r = np.ascontiguousarray(lens["radius"], np.float32)
        t = np.ascontiguousarray(lens["thickness"], np.float32)
        i = np.ascontiguousarray(lens["ior"], np.float32)
        h = np.ascontiguousarray(lens["semi_aperture"], np.float32)
        self._ck(self.lib.lf_set_lens(self.ctx, int(lens["n"]), int(lens["stop"]), int(i.shape[0]),
                                      _fp(r, C.c_float), _fp(t, C.c_float), _fp(i, C.c_float),
                                      _fp(h, C.c_float), C.c_float(lens["sensor_width_mm"])))
        if "coatings" in lens:
            c = lens["coatings"]
            self.set_lens_coatings(c["lambda_nm"], c["thickness_nm"], c["index"])
        if "coating_stacks" in lens:
            c = lens["coating_stacks"]
            self.set_lens_coating_stacks(c["lambda_nm"], c["n_layers"], c["thickness_nm"], c["index"])
        if "aspheres" in lens:
            self.set_lens_aspheres(lens["aspheres"]["conic"], lens["aspheres"]["coef"])
        if "biconics" in lens:
            b = lens["biconics"]
            self.set_lens_biconics(b["on"], b["radius_x"], b["conic_x"], b["conic_y"])
        if "poses" in lens:
            p = lens["poses"]
            self.set_lens_poses(p["on"], p["decentre"], p["tilt_deg"])
        if "sensor_reflectance" in lens:
            self.set_sensor_reflectance(lens["sensor_reflectance"])

    def set_sensor_reflectance(self, reflectance=None):
        """The sensor's reflectance, one value in [0, 1] per index column of the installed lens (None clears it)."""
        if reflectance is None:
            self._ck(self.lib.lf_set_sensor_reflectance(self.ctx, 0, None))
            return
        r = np.ascontiguousarray(reflectance, np.float32).ravel()
        self._ck(self.lib.lf_set_sensor_reflectance(self.ctx, len(r), _fp(r, C.c_float)))

    def sensor_reflectance(self):
        """The installed reflectance per index column, or None."""
        nl = self.lens_info()["n_lambda"]
        r = np.zeros(nl, np.float32)
        on = C.c_int()
        self._ck(self.lib.lf_get_sensor_reflectance(self.ctx, nl, _fp(r, C.c_float), C.byref(on)))
        return r if on.value else None

    def set_sensor_ghosts(self, mode=SENSOR_GHOSTS_ADD, interfaces=None):
        """Sensor-reflection ghosts: SENSOR_GHOSTS_OFF / _ADD (behind the ordinary march) / _ONLY; interfaces None: every
        interface but the stop."""
        if interfaces is None:
            self._ck(self.lib.lf_set_sensor_ghosts(self.ctx, int(mode), None, 0))
            return
        sel = np.ascontiguousarray(interfaces, np.int32).ravel()
        self._ck(self.lib.lf_set_sensor_ghosts(self.ctx, int(mode), _fp(sel, C.c_int), len(sel)))

    def sensor_ghosts(self):
        """(mode, the interfaces a launch marches)"""
        mode, n = C.c_int(), C.c_int()
        sel = np.zeros(16, np.int32)
        self._ck(self.lib.lf_get_sensor_ghosts(self.ctx, C.byref(mode), _fp(sel, C.c_int), len(sel), C.byref(n)))
        return mode.value, [int(v) for v in sel[:n.value]]

    def set_sensor_ghost_surfaces(self, which=SENSOR_SURFACES_POSED):
        """Which interfaces a sensor path may meet: SENSOR_SURFACES_CENTRED (the default: a lens with pose records is refused)
        or SENSOR_SURFACES_POSED (trace_ghosts under SENSOR_GHOSTS_ADD / _ONLY and march_sensor_path_rays march it).  A
        setting of the context: set_lens and focus_lens keep it; a lens without pose records renders the same bits under both."""
        self._ck(self.lib.lf_set_sensor_ghost_surfaces(self.ctx, int(which)))

    def sensor_ghost_surfaces(self):
        which = C.c_int()
        self._ck(self.lib.lf_get_sensor_ghost_surfaces(self.ctx, C.byref(which)))
        return which.value

    def march_sensor_path_rays(self, lam, i, sensor_xy_mm, pupil_uv):
        """march_path_rays along the sensor path of interface i: n x 8, the weight with the sensor's reflectance."""
        xy = np.ascontiguousarray(sensor_xy_mm, np.float32).reshape(-1, 2)
        uv = np.ascontiguousarray(pupil_uv, np.float32).reshape(-1, 2)
        out = np.zeros((len(xy), 8), np.float32)
        self._ck(self.lib.lf_march_sensor_path_rays(self.ctx, int(lam), int(i), C.c_size_t(len(xy)), _fp(xy, C.c_float),
                                                    _fp(uv, C.c_float), _fp(out, C.c_float)))
        return out

    def sensor_path_sequence(self, i):
        """sensor_path_sequence of the installed lens"""
        info = self.lens_info()
        return sensor_path_sequence(info["n"], info["stop"], i)

    def sensor_ghost_stats(self):
        """{started, reached_sensor, lost_at_sensor, lit} of the sensor paths since reset_counters"""
        out = (C.c_uint64 * 4)()
        self._ck(self.lib.lf_get_sensor_ghost_stats(self.ctx, out))
        return dict(zip(("started", "reached_sensor", "lost_at_sensor", "lit"), (int(v) for v in out)))

    def set_lens_biconics(self, on=None, radius_x=None, conic_x=None, conic_y=None):
        """Biconic records on the installed lens: on[k] != 0 marks interface k, radius_x[k] its x-meridian radius (0: flat in
        x), conic_x[k] / conic_y[k] its conic constants (None: zeros).  on None clears the records."""
        if on is None:
            self._ck(self.lib.lf_set_lens_biconics(self.ctx, 0, None, None, None, None))
            return
        on = np.ascontiguousarray(on, np.int32).ravel()
        arr = lambda v: np.zeros(len(on), np.float32) if v is None else np.ascontiguousarray(v, np.float32).ravel()
        rx, kx, ky = arr(radius_x), arr(conic_x), arr(conic_y)
        if not (len(rx) == len(kx) == len(ky) == len(on)):
            raise ValueError("on, radius_x, conic_x and conic_y hold one value per interface")
        self._ck(self.lib.lf_set_lens_biconics(self.ctx, len(on), _fp(on, C.c_int), _fp(rx, C.c_float), _fp(kx, C.c_float),
                                               _fp(ky, C.c_float)))

    def lens_biconics(self):
        """dict(on, radius_x, conic_x, conic_y (n each), n_biconic) of the installed lens."""
        n = self.lens_info()["n"]
        on = np.zeros(n, np.int32)
        rx, kx, ky = (np.zeros(n, np.float32) for _ in range(3))
        cnt = C.c_int()
        self._ck(self.lib.lf_get_lens_biconics(self.ctx, n, _fp(on, C.c_int), _fp(rx, C.c_float), _fp(kx, C.c_float),
                                               _fp(ky, C.c_float), C.byref(cnt)))
        return dict(on=on, radius_x=rx, conic_x=kx, conic_y=ky, n_biconic=cnt.value)

    def set_lens_poses(self, on=None, decentre=None, tilt_deg=None):
        """Pose records on the installed lens: on[k] != 0 marks interface k, decentre[k] = (dx, dy, dz) in mm, tilt_deg[k] =
        (ax, ay, az) in degrees (None: zeros).  on None clears the records.  (pose_group writes a rigid group's.)"""
        if on is None:
            self._ck(self.lib.lf_set_lens_poses(self.ctx, 0, None, None, None))
            return
        on = np.ascontiguousarray(on, np.int32).ravel()
        arr = lambda v: np.zeros((len(on), 3), np.float32) if v is None else np.ascontiguousarray(v, np.float32).reshape(-1, 3)
        d, t = arr(decentre), arr(tilt_deg)
        if not (len(d) == len(t) == len(on)):
            raise ValueError("on holds one value per interface, decentre and tilt_deg three")
        self._ck(self.lib.lf_set_lens_poses(self.ctx, len(on), _fp(on, C.c_int), _fp(d, C.c_float), _fp(t, C.c_float)))

    def lens_poses(self):
        """dict(on (n), decentre, tilt_deg (n x 3 each), n_posed) of the installed lens."""
        n = self.lens_info()["n"]
        on = np.zeros(n, np.int32)
        d, t = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        cnt = C.c_int()
        self._ck(self.lib.lf_get_lens_poses(self.ctx, n, _fp(on, C.c_int), _fp(d, C.c_float), _fp(t, C.c_float), C.byref(cnt)))
        return dict(on=on, decentre=d, tilt_deg=t, n_posed=cnt.value)

    def pose_events(self, curvature_x, curvature_y, conic_x, conic_y, asphere, decentre, tilt_deg, semi_aperture, n_in, n_out,
                    reflect, forward, dzv, rays):
        """pose_event on the device (lf_pose_events): the same (out, fates), bit for bit."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((len(rays), 8), np.float32)
        fates = np.zeros(len(rays), np.int32)
        keep, consts = _pose_event_consts(curvature_x, curvature_y, conic_x, conic_y, asphere, decentre, tilt_deg, semi_aperture,
                                          n_in, n_out, reflect, forward, dzv)
        self._ck(self.lib.lf_pose_events(self.ctx, *consts, C.c_size_t(len(rays)), _fp(rays, C.c_float), _fp(out, C.c_float),
                                         _fp(fates, C.c_int)))
        return out, fates

    def lens_meridian_scales(self):
        """(scale_x, scale_y): the paraxial image scales of the x and the y meridian (lf_get_lens_meridian_scales)."""
        sx, sy = C.c_double(), C.c_double()
        self._ck(self.lib.lf_get_lens_meridian_scales(self.ctx, C.byref(sx), C.byref(sy)))
        return sx.value, sy.value

    def biconic_events(self, curvature_x, curvature_y, conic_x, conic_y, semi_aperture, n_in, n_out, reflect, forward, dzv, rays):
        """biconic_event on the device (lf_biconic_events): the same (out, fates), bit for bit."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((len(rays), 8), np.float32)
        fates = np.zeros(len(rays), np.int32)
        self._ck(self.lib.lf_biconic_events(self.ctx, C.c_float(curvature_x), C.c_float(curvature_y), C.c_float(conic_x),
                                            C.c_float(conic_y), C.c_float(semi_aperture), C.c_float(n_in), C.c_float(n_out),
                                            int(bool(reflect)), int(bool(forward)), C.c_float(dzv), C.c_size_t(len(rays)),
                                            _fp(rays, C.c_float), _fp(out, C.c_float), _fp(fates, C.c_int)))
        return out, fates

    def set_lens_aspheres(self, conic=None, coef=None):
        """Conic constants conic[k] and even coefficients coef[m, k] (A4, A6, ... of interface k; up to MAX_ASPH_COEF rows)
        on the installed lens.  conic None clears the aspheres."""
        if conic is None:
            self._ck(self.lib.lf_set_lens_aspheres(self.ctx, 0, None, 0, None))
            return
        kap = np.ascontiguousarray(conic, np.float32).ravel()
        a = np.zeros((0, len(kap)), np.float32) if coef is None else np.atleast_2d(np.asarray(coef, np.float32))
        if a.shape[1:] != (len(kap),):
            raise ValueError("coef is (n_coef, n_surfaces)")
        a = np.ascontiguousarray(a)
        self._ck(self.lib.lf_set_lens_aspheres(self.ctx, len(kap), _fp(kap, C.c_float), int(a.shape[0]),
                                               _fp(a, C.c_float) if a.shape[0] else None))

    def lens_aspheres(self):
        """dict(conic (n), coef (MAX_ASPH_COEF x n), n_aspheric) of the installed lens."""
        n = self.lens_info()["n"]
        kap = np.zeros(n, np.float32)
        a = np.zeros((MAX_ASPH_COEF, n), np.float32)
        cnt = C.c_int()
        self._ck(self.lib.lf_get_lens_aspheres(self.ctx, n, _fp(kap, C.c_float), _fp(a, C.c_float), C.byref(cnt)))
        return dict(conic=kap, coef=a, n_aspheric=cnt.value)

    def asphere_events(self, curvature, conic, coef, semi_aperture, n_in, n_out, reflect, forward, dzv, rays):
        """asphere_event on the device (lf_asphere_events): the same (out, fates), bit for bit."""
        a = np.ascontiguousarray(coef, np.float32).ravel()
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((len(rays), 8), np.float32)
        fates = np.zeros(len(rays), np.int32)
        self._ck(self.lib.lf_asphere_events(self.ctx, C.c_float(curvature), C.c_float(conic), len(a), _fp(a, C.c_float),
                                            C.c_float(semi_aperture), C.c_float(n_in), C.c_float(n_out), int(bool(reflect)),
                                            int(bool(forward)), C.c_float(dzv), C.c_size_t(len(rays)), _fp(rays, C.c_float),
                                            _fp(out, C.c_float), _fp(fates, C.c_int)))
        return out, fates

    def march_path_rays(self, lam, i, j, sensor_xy_mm, pupil_uv):
        """generate_lens_rays along the ghost path of pair (i, j) ((-1, -1): the primary path): n x 8."""
        xy = np.ascontiguousarray(sensor_xy_mm, np.float32).reshape(-1, 2)
        uv = np.ascontiguousarray(pupil_uv, np.float32).reshape(-1, 2)
        out = np.zeros((len(xy), 8), np.float32)
        self._ck(self.lib.lf_march_path_rays(self.ctx, int(lam), int(i), int(j), C.c_size_t(len(xy)), _fp(xy, C.c_float),
                                             _fp(uv, C.c_float), _fp(out, C.c_float)))
        return out

    def set_lens_coating_stacks(self, lambda_nm, n_layers=None, thickness_nm=None, index=None):
        """Stacks of layers on the installed lens: lambda_nm[l], n_layers[k] (0 = bare), thickness_nm[j, k] and
        index[j, l, k] of layer j (0 = the scene side) of interface k; j runs over max(n_layers) layers or more.
        n_layers None clears every stack."""
        if n_layers is None:
            self._ck(self.lib.lf_set_lens_coating_stacks(self.ctx, 0, 0, None, None, None, None))
            return
        lam = np.ascontiguousarray(lambda_nm, np.float32).ravel()
        nl = np.ascontiguousarray(n_layers, np.int32).ravel()
        d = np.atleast_2d(np.asarray(thickness_nm, np.float32))
        m = np.asarray(index, np.float32)
        if m.ndim == 2:              # one index per layer and interface, for every wavelength
            m = np.repeat(m[:, None, :], len(lam), axis=1)
        if d.shape[1:] != (len(nl),) or m.shape != (d.shape[0], len(lam), len(nl)):
            raise ValueError("thickness_nm is (layers, n_surfaces), index (layers, n_lambda, n_surfaces)")
        # (the arrays always hold MAX_COAT_LAYERS layers: a count beyond that is the library's to refuse)
        rows = max(MAX_COAT_LAYERS, d.shape[0], int(nl.max()) if len(nl) else 0)
        d = np.ascontiguousarray(np.concatenate([d, np.zeros((rows - d.shape[0], len(nl)), np.float32)]))
        m = np.ascontiguousarray(np.concatenate([m, np.zeros((rows - m.shape[0], len(lam), len(nl)), np.float32)]))
        self._ck(self.lib.lf_set_lens_coating_stacks(self.ctx, len(nl), len(lam), _fp(lam, C.c_float), _fp(nl, C.c_int),
                                                     _fp(d, C.c_float), _fp(m, C.c_float)))

    def get_lens_coating_stacks(self):
        """dict(lambda_nm, n_layers, thickness_nm (MAX_COAT_LAYERS x n), index (MAX_COAT_LAYERS x n_lambda x n), n_stacked)
        of the installed lens, after the drop of zero-thickness layers."""
        info = self.lens_info()
        n, nl = info["n"], info["n_lambda"]
        lam = np.zeros(nl, np.float32)
        cnt = np.zeros(n, np.int32)
        d = np.zeros((MAX_COAT_LAYERS, n), np.float32)
        m = np.zeros((MAX_COAT_LAYERS, nl, n), np.float32)
        ns = C.c_int()
        self._ck(self.lib.lf_get_lens_coating_stacks(self.ctx, n, nl, _fp(lam, C.c_float), _fp(cnt, C.c_int),
                                                     _fp(d, C.c_float), _fp(m, C.c_float), C.byref(ns)))
        return dict(lambda_nm=lam, n_layers=cnt, thickness_nm=d, index=m, n_stacked=ns.value)

    def set_lens_coatings(self, lambda_nm, thickness_nm=None, index=None):
        """Single-layer films on the installed lens: lambda_nm[l] (the index columns' wavelengths), thickness_nm[k]
        (0 = bare), index[l, k] (n_lambda x n_surfaces, or one value per interface / one for all).
        thickness_nm None clears every coating."""
        if thickness_nm is None:
            self._ck(self.lib.lf_set_lens_coatings(self.ctx, 0, 0, None, None, None))
            return
        lam = np.ascontiguousarray(lambda_nm, np.float32).ravel()
        d = np.ascontiguousarray(thickness_nm, np.float32).ravel()
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(index, np.float32), (len(lam), len(d))), np.float32)
        self._ck(self.lib.lf_set_lens_coatings(self.ctx, len(d), len(lam), _fp(lam, C.c_float), _fp(d, C.c_float),
                                               _fp(m, C.c_float)))

    def lens_coatings(self):
        """dict(lambda_nm, thickness_nm, index (n_lambda x n), n_coated) of the installed lens."""
        info = self.lens_info()
        n, nl = info["n"], info["n_lambda"]
        lam = np.zeros(nl, np.float32)
        d = np.zeros(n, np.float32)
        m = np.zeros((nl, n), np.float32)
        nc = C.c_int()
        self._ck(self.lib.lf_get_lens_coatings(self.ctx, n, nl, _fp(lam, C.c_float), _fp(d, C.c_float),
                                               _fp(m, C.c_float), C.byref(nc)))
        return dict(lambda_nm=lam, thickness_nm=d, index=m, n_coated=nc.value)

    def set_lambda_rgb(self, weights):
        w = np.ascontiguousarray(weights, np.float32)
        self._ck(self.lib.lf_set_lambda_rgb(self.ctx, _fp(w, C.c_float)))

    def set_sun(self, direction, radiance, angular_radius):
        d = np.ascontiguousarray(direction, np.float32)
        r = np.ascontiguousarray(radiance, np.float32)
        self._ck(self.lib.lf_set_sun(self.ctx, _fp(d, C.c_float), _fp(r, C.c_float),
                                     C.c_float(angular_radius)))

    def set_sun_from_flares(self, flare=0, efl_mm=0.0, angular_radius=0.05):
        self._ck(self.lib.lf_set_sun_from_flares(self.ctx, int(flare), C.c_double(efl_mm),
                                                 C.c_float(angular_radius)))

    def set_lights(self, directions, radiances, angular_radii):
        """Several lights in ONE pass of the march (lf_set_lights): n x 3 directions (z < 0), n x 3 radiances, n angular
        radii, 1 <= n <= MAX_LIGHTS.  Replaces all lights; a refusal leaves the previous ones.  The frame is the sum of
        the n single-light frames, bit for bit."""
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(radiances, np.float32).reshape(-1, 3)
        a = np.ascontiguousarray(angular_radii, np.float32).reshape(-1)
        if not (len(d) == len(r) == len(a)):
            raise ValueError("set_lights: one direction, one radiance and one angular radius per light")
        self._ck(self.lib.lf_set_lights(self.ctx, len(d), _fp(d, C.c_float), _fp(r, C.c_float), _fp(a, C.c_float)))

    def lights(self):
        """(directions n x 3 as stored, radiances n x 3, angular radii n) of the installed lights (lf_get_lights)"""
        n = C.c_int(0)
        d = np.zeros((MAX_LIGHTS, 3), np.float32)
        r = np.zeros((MAX_LIGHTS, 3), np.float32)
        a = np.zeros(MAX_LIGHTS, np.float32)
        self._ck(self.lib.lf_get_lights(self.ctx, C.byref(n), _fp(d, C.c_float), _fp(r, C.c_float), _fp(a, C.c_float)))
        return d[:n.value].copy(), r[:n.value].copy(), a[:n.value].copy()

    def set_lights_from_flares(self, efl_mm=0.0, angular_radius=0.05):
        """every in-frame flare of the flare state becomes a light of the march (lf_set_lights_from_flares); returns how many"""
        n = C.c_int(0)
        self._ck(self.lib.lf_set_lights_from_flares(self.ctx, C.c_double(efl_mm), C.c_float(angular_radius), C.byref(n)))
        return n.value

    # ---- lights at a finite distance (lf_set_lights_ex)
    def set_lights_ex(self, kinds, vecs, radiances, angular_radii):
        """Lights of mixed kinds in one pass of the march (lf_set_lights_ex): per light LIGHT_DIRECTIONAL with a direction
        (z < 0) or LIGHT_POINT with a position in lens millimetres (front vertex at z = 0, the scene at z < 0; not closer
        than the front element's limits).  Replaces all lights; a refusal leaves the previous ones."""
        k = np.ascontiguousarray(kinds, np.int32).reshape(-1)
        v = np.ascontiguousarray(vecs, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(radiances, np.float32).reshape(-1, 3)
        a = np.ascontiguousarray(angular_radii, np.float32).reshape(-1)
        if not (len(k) == len(v) == len(r) == len(a)):
            raise ValueError("set_lights_ex: one kind, one vector, one radiance and one angular radius per light")
        self._ck(self.lib.lf_set_lights_ex(self.ctx, len(k), _fp(k, C.c_int), _fp(v, C.c_float), _fp(r, C.c_float),
                                           _fp(a, C.c_float)))

    def lights_ex(self):
        """(kinds n, vectors n x 3 -- direction or position as stored --, radiances n x 3, angular radii n) (lf_get_lights_ex)"""
        n = C.c_int(0)
        k = np.zeros(MAX_LIGHTS, np.int32)
        v = np.zeros((MAX_LIGHTS, 3), np.float32)
        r = np.zeros((MAX_LIGHTS, 3), np.float32)
        a = np.zeros(MAX_LIGHTS, np.float32)
        self._ck(self.lib.lf_get_lights_ex(self.ctx, C.byref(n), _fp(k, C.c_int), _fp(v, C.c_float), _fp(r, C.c_float),
                                           _fp(a, C.c_float)))
        return k[:n.value].copy(), v[:n.value].copy(), r[:n.value].copy(), a[:n.value].copy()

    def set_lights_from_scene(self, efl_mm=0.0, angular_radius=0.05, world_per_mm=0.001):
        """the in-frame flares and the scene's PointLights become the lights of the march (lf_set_lights_from_scene);
        returns (directional, point) lights installed"""
        nd, npt = C.c_int(0), C.c_int(0)
        self._ck(self.lib.lf_set_lights_from_scene(self.ctx, C.c_double(efl_mm), C.c_float(angular_radius),
                                                   C.c_double(world_per_mm), C.byref(nd), C.byref(npt)))
        return nd.value, npt.value

    # ---- area lights (lf_set_lights_geom)
    def set_lights_geom(self, kinds, geoms, radiances, angular_radii):
        """Lights of all three kinds (lf_set_lights_geom): 12 floats per light -- kinds 0 and 1 the vector of set_lights_ex in
        the first three, LIGHT_AREA centre, direction, dim_x, dim_y in lens millimetres.  Replaces all lights."""
        k = np.ascontiguousarray(kinds, np.int32).reshape(-1)
        g = np.ascontiguousarray([_geom(x) for x in geoms], np.float32).reshape(-1, LIGHT_GEOM_FLOATS)
        r = np.ascontiguousarray(radiances, np.float32).reshape(-1, 3)
        a = np.ascontiguousarray(angular_radii, np.float32).reshape(-1)
        if not (len(k) == len(g) == len(r) == len(a)):
            raise ValueError("set_lights_geom: one kind, one geometry, one radiance and one angular radius per light")
        self._ck(self.lib.lf_set_lights_geom(self.ctx, len(k), _fp(k, C.c_int), _fp(g, C.c_float), _fp(r, C.c_float),
                                             _fp(a, C.c_float)))

    def lights_geom(self):
        """(kinds n, geometry n x 12 as stored, radiances n x 3, angular radii n) (lf_get_lights_geom)"""
        n = C.c_int(0)
        k = np.zeros(MAX_LIGHTS, np.int32)
        g = np.zeros((MAX_LIGHTS, LIGHT_GEOM_FLOATS), np.float32)
        r = np.zeros((MAX_LIGHTS, 3), np.float32)
        a = np.zeros(MAX_LIGHTS, np.float32)
        self._ck(self.lib.lf_get_lights_geom(self.ctx, C.byref(n), _fp(k, C.c_int), _fp(g, C.c_float), _fp(r, C.c_float),
                                             _fp(a, C.c_float)))
        return k[:n.value].copy(), g[:n.value].copy(), r[:n.value].copy(), a[:n.value].copy()

    def set_lights_from_scene_ex(self, efl_mm=0.0, angular_radius=0.05, world_per_mm=0.001):
        """set_lights_from_scene plus the scene's AreaLights (lf_set_lights_from_scene_ex); returns (directional, point,
        area) lights installed"""
        nd, npt, na = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self.lib.lf_set_lights_from_scene_ex(self.ctx, C.c_double(efl_mm), C.c_float(angular_radius),
                                                      C.c_double(world_per_mm), C.byref(nd), C.byref(npt), C.byref(na)))
        return nd.value, npt.value, na.value

    def ghost_ray_light_factors(self, rays):
        """rays: n x 6 (origin xyz in lens millimetres, z absolute; direction xyz).  Returns n x n_lights float32: (1 - q_k)^2
        where ray i lies inside installed light k, 0 elsewhere (the lit epilogue's own test, lf_ghost_ray_light_factors)."""
        r = np.asarray(rays)
        if r.ndim != 2 or r.shape[1] != 6:
            raise ValueError("ghost_ray_light_factors: rays must be n x 6 (origin xyz in lens mm, direction xyz)")
        r = np.ascontiguousarray(r, np.float32)
        if not np.isfinite(r).all():
            raise ValueError("ghost_ray_light_factors: rays must be finite")
        n = C.c_int(0)
        self._ck(self.lib.lf_get_lights(self.ctx, C.byref(n), None, None, None))
        out = np.zeros((len(r), max(1, n.value)), np.float32)
        self._ck(self.lib.lf_ghost_ray_light_factors(self.ctx, C.c_size_t(len(r)), _fp(r, C.c_float), _fp(out, C.c_float)))
        return out[:, :n.value]

    # ---- ghost occlusion (lf_set_ghost_occlusion): a light's ghosts hidden behind the scene
    def set_ghost_occlusion(self, on=True, world_per_mm=0.001):
        """On: a lit ghost ray adds only what the scene does not block -- its own exit point on the front element along
        its own exit direction, mapped to the world as the lens camera maps it (world_per_mm scene units per lens
        millimetre, > 0 and finite).  Off (the default): the launch is the one it always was.  trace_ghosts then needs
        a lens, set_camera and a scene."""
        on = bool(on)
        w = float(world_per_mm)
        if on and not (w > 0.0 and np.isfinite(w)):
            raise ValueError("set_ghost_occlusion: world_per_mm must be > 0 and finite")
        self._ck(self.lib.lf_set_ghost_occlusion(self.ctx, int(on), C.c_double(w)))

    def get_ghost_occlusion(self):
        """dict(on, world_per_mm, march_variant): the setting, and the kernel variant the next launch takes (bit value
        16 = the occlusion kernels)"""
        on, w, v = C.c_int(0), C.c_double(0.0), C.c_int(0)
        self._ck(self.lib.lf_get_ghost_occlusion(self.ctx, C.byref(on), C.byref(w), C.byref(v)))
        return dict(on=bool(on.value), world_per_mm=w.value, march_variant=v.value)

    def ghost_occlusion_stats(self):
        """dict(tested, blocked): (ray, light) shadow tests made since reset_counters, and how many of them were blocked"""
        out = (C.c_uint64 * 2)()
        self._ck(self.lib.lf_get_ghost_occlusion_stats(self.ctx, out))
        return dict(tested=int(out[0]), blocked=int(out[1]))

    def ghost_ray_visibility(self, rays):
        """rays: n x 6 (origin xyz in lens millimetres, direction xyz).  Returns n bools: would the exit ray see the sky
        (the mapping and the any-hit walk of the march's shadow rays, on the state installed)."""
        r = np.asarray(rays)
        if r.ndim != 2 or r.shape[1] != 6:
            raise ValueError("ghost_ray_visibility: rays must be n x 6 (origin xyz in lens mm, direction xyz)")
        r = np.ascontiguousarray(r, np.float32)
        if not np.isfinite(r).all() or not (np.abs(r[:, 3:]).max(axis=1) > 0.0).all():
            raise ValueError("ghost_ray_visibility: rays must be finite, directions non-zero")
        vis = np.zeros(len(r), np.uint8)
        self._ck(self.lib.lf_ghost_ray_visibility(self.ctx, C.c_size_t(len(r)), _fp(r, C.c_float),
                                                  vis.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return vis.astype(bool)

    # ---- flare occlusion (lf_set_flare_occlusion): the starburst, the falloff and the paraxial quads of a blocked light
    def set_flare_occlusion(self, on=True, rays_per_light=1024, angular_radius=0.00465, origin=FLARE_ORIGIN_CAMERA,
                            world_per_mm=0.001):
        """On: render_flare_layer, irradiance_falloff and generate_ghost_buffer scale each flare by the fraction of its
        rays_per_light shadow rays (over the light's disc of angular_radius, from the camera position or over the front
        element) that the resident scene does not block.  Off (the default): the launches are the ones they always were.
        While on, those calls need set_camera and a scene (and a lens under FLARE_ORIGIN_FRONT_ELEMENT)."""
        if not bool(on):
            self._ck(self.lib.lf_set_flare_occlusion(self.ctx, 0, 0, C.c_float(0.0), 0, C.c_double(0.0)))
            return
        R, a, origin = _flare_occlusion_args("set_flare_occlusion", rays_per_light, angular_radius, origin, world_per_mm)
        self._ck(self.lib.lf_set_flare_occlusion(self.ctx, 1, R, C.c_float(a), origin, C.c_double(float(world_per_mm))))

    def get_flare_occlusion(self):
        """dict(on, rays_per_light, angular_radius, origin, world_per_mm)"""
        on, R, a, o, w = C.c_int(0), C.c_int(0), C.c_float(0.0), C.c_int(0), C.c_double(0.0)
        self._ck(self.lib.lf_get_flare_occlusion(self.ctx, C.byref(on), C.byref(R), C.byref(a), C.byref(o), C.byref(w)))
        return dict(on=bool(on.value), rays_per_light=R.value, angular_radius=a.value, origin=o.value, world_per_mm=w.value)

    def flare_visibility(self):
        """dict(n, visibility float64[n], visible_rays uint64[n]) of the flare state installed, computed now"""
        n = C.c_int(0)
        vis, cnt = np.zeros(MAX_FLARES, np.float64), np.zeros(MAX_FLARES, np.uint64)
        self._ck(self.lib.lf_get_flare_visibility(self.ctx, C.byref(n), _fp(vis, C.c_double), _fp(cnt, C.c_uint64)))
        return dict(n=n.value, visibility=vis[:n.value].copy(), visible_rays=cnt[:n.value].copy())

    def set_ghost_occlusion_reach(self, reach):
        """Where the shadow ray of a POINT light ends: OCCLUSION_REACH_SKY (the default: the ray runs on to the sky, and occlusion
        with a point light installed is refused) or OCCLUSION_REACH_LIGHT (it ends at the point of the ray nearest the lamp: a
        wall behind the lamp does not hide it).  A setting of the context; no effect while occlusion is off, none on
        directional lights."""
        if isinstance(reach, bool) or not isinstance(reach, (int, np.integer)) or int(reach) not in (OCCLUSION_REACH_SKY, OCCLUSION_REACH_LIGHT):
            raise ValueError("set_ghost_occlusion_reach: OCCLUSION_REACH_SKY (0) or OCCLUSION_REACH_LIGHT (1)")
        self._ck(self.lib.lf_set_ghost_occlusion_reach(self.ctx, int(reach)))

    def get_ghost_occlusion_reach(self):
        reach = C.c_int(0)
        self._ck(self.lib.lf_get_ghost_occlusion_reach(self.ctx, C.byref(reach)))
        return reach.value

    def ghost_ray_light_visibility(self, rays):
        """rays: n x 6 (origin xyz in lens millimetres, direction xyz).  Returns n x n_lights bools: does ray i's shadow ray find
        nothing over [0, reach_k] -- to the sky for a directional light, to the lamp for a point light (the mapping, reach and
        any-hit walk of the march's shadow rays, on the state installed; whether or not the ray lies in lobe k)."""
        r = np.asarray(rays)
        if r.ndim != 2 or r.shape[1] != 6:
            raise ValueError("ghost_ray_light_visibility: rays must be n x 6 (origin xyz in lens mm, direction xyz)")
        r = np.ascontiguousarray(r, np.float32)
        if not np.isfinite(r).all() or not (np.abs(r[:, 3:]).max(axis=1) > 0.0).all():
            raise ValueError("ghost_ray_light_visibility: rays must be finite, directions non-zero")
        n = C.c_int(0)
        self._ck(self.lib.lf_get_lights(self.ctx, C.byref(n), None, None, None))
        vis = np.zeros((len(r), max(1, n.value)), np.uint8)
        self._ck(self.lib.lf_ghost_ray_light_visibility(self.ctx, C.c_size_t(len(r)), _fp(r, C.c_float),
                                                        vis.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return vis[:, :n.value].astype(bool)

    def set_ghost_pairs(self, pairs=None, include_primary=True):
        if pairs is None or len(pairs) == 0:
            self._ck(self.lib.lf_set_ghost_pairs(self.ctx, None, 0, int(include_primary)))
        else:
            p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
            self._ck(self.lib.lf_set_ghost_pairs(self.ctx, _fp(p, C.c_int), len(p),
                                                 int(include_primary)))

    def set_pupil_subcells(self, bits):
        self._ck(self.lib.lf_set_pupil_subcells(self.ctx, int(bits)))

    def set_tile_stride(self, stride):
        self._ck(self.lib.lf_set_tile_stride(self.ctx, int(stride)))

    def trace_ghosts(self, spp, key=0x1e45f1a4e):
        self._ck(self.lib.lf_trace_ghosts(self.ctx, int(spp), C.c_uint64(key)))

    def set_march_culling(self, mode=1):
        """0 = every sample marches every path (rounds 1-4), 1 = start only the paths that can reach the light
        (default), 2 = the same with the cull table rebuilt at every launch."""
        self._ck(self.lib.lf_set_march_culling(self.ctx, int(mode)))

    def cull_info(self):
        v = (C.c_int * 8)()
        self._ck(self.lib.lf_get_cull_info(self.ctx, v))
        return dict(mode=v[0], culled=bool(v[1]), blocks_x=v[2], blocks_y=v[3], cells=v[4], G=v[5], P=v[6], block_px=v[7],
                    reason=self.cull_reason())

    CULL_REASONS = ("applied", "off", "no_stop", "too_many_paths", "too_many_samples", "block_too_large", "table_too_full",
                    "audit_refuted", "dispersion_not_monotonic", "aspheric", "anamorphic", "posed")

    def cull_reason(self):
        """why the last trace_ghosts did (not) cull: one of CULL_REASONS (lf_cull_reason)"""
        r = C.c_int()
        self._ck(self.lib.lf_get_cull_reason(self.ctx, C.byref(r)))
        return self.CULL_REASONS[r.value]

    def set_cull_audit(self, rays_per_dropped_box=1):
        """rays marched per (block, cell, path) combination the cull table does not start (0 = no audit)"""
        self._ck(self.lib.lf_set_cull_audit(self.ctx, int(rays_per_dropped_box)))

    def cull_audit(self):
        """{rays, lit, launches_refuted} since reset_counters: the audit of what the cull tables dropped"""
        r, l, n = C.c_uint64(), C.c_uint64(), C.c_int()
        self._ck(self.lib.lf_get_cull_audit(self.ctx, C.byref(r), C.byref(l), C.byref(n)))
        return dict(rays=r.value, lit=l.value, launches_refuted=n.value)

    def test_knob(self, name, value):
        """TEST HOOK (lensflare.h lf_test_knob): the suite's and the bench's A/B switches, by name"""
        self._ck(self.lib.lf_test_knob(self.ctx, name.encode(), C.c_double(float(value))))

    def cull_started_fraction(self):
        f = C.c_double(0.0)
        self._ck(self.lib.lf_get_cull_started_fraction(self.ctx, C.byref(f)))
        return f.value

    # ---- the pre-pass of a multi-GPU frame, shared (include/lensflare.h)
    def comm_share_cull(self, on=True):
        self._ck(self.lib.lf_comm_share_cull(self.ctx, int(bool(on))))

    def set_cull_share(self, rank, nranks):
        self._ck(self.lib.lf_set_cull_share(self.ctx, int(rank), int(nranks)))

    def cull_prepare(self, spp):
        self._ck(self.lib.lf_cull_prepare(self.ctx, int(spp)))

    def cull_table_view(self):
        """(device pointer, entries, entries per rank) of the table the host completes; (0, 0, 0): this launch does not cull"""
        p, n, k = C.c_void_p(), C.c_uint64(), C.c_uint64()
        self._ck(self.lib.lf_cull_table_view(self.ctx, C.byref(p), C.byref(n), C.byref(k)))
        return p.value or 0, n.value, k.value

    def cull_commit(self):
        self._ck(self.lib.lf_cull_commit(self.ctx))

    def cull_table(self):
        """The path masks of the last trace_ghosts, (blocks_y, blocks_x, cells + 1) uint64; None if it did not cull."""
        i = self.cull_info()
        if not i["culled"]:
            return None
        t = np.zeros((i["blocks_y"], i["blocks_x"], i["cells"] + 1), np.uint64)
        self._ck(self.lib.lf_get_cull_table(self.ctx, _fp(t, C.c_uint64), C.c_size_t(t.size)))
        return t

    def cull_table_and_block(self):
        """(table, block side in pixels) for a checker that follows the device's table; None if not culled."""
        t = self.cull_table()
        return None if t is None else (t, self.cull_info()["block_px"])

    def march_fix_bits(self):
        b = C.c_int(0)
        self._ck(self.lib.lf_get_march_fix_bits(self.ctx, C.byref(b)))
        return b.value

    def generate_lens_rays(self, lam, sensor_xy_mm, pupil_uv):
        xy = np.ascontiguousarray(sensor_xy_mm, np.float32).reshape(-1, 2)
        uv = np.ascontiguousarray(pupil_uv, np.float32).reshape(-1, 2)
        out = np.zeros((len(xy), 8), np.float32)
        self._ck(self.lib.lf_generate_lens_rays(self.ctx, int(lam), C.c_size_t(len(xy)),
                                                _fp(xy, C.c_float), _fp(uv, C.c_float),
                                                _fp(out, C.c_float)))
        return out

    def counters(self):
        c = Counters()
        self._ck(self.lib.lf_get_counters(self.ctx, C.byref(c)))
        return c.as_dict()

    def set_starburst_spectrum(self, scale=None, rgb_weights=None):
        """Row f4: per-wavelength starburst; None / empty = the reference's monochrome starburst."""
        if scale is None or len(scale) == 0:
            self._ck(self.lib.lf_set_starburst_spectrum(self.ctx, 0, None, None))
            return
        sc = np.ascontiguousarray(scale, np.float64).ravel()
        w = np.ascontiguousarray(rgb_weights, np.float64).reshape(len(sc), 3)
        self._ck(self.lib.lf_set_starburst_spectrum(self.ctx, len(sc), _fp(sc, C.c_double),
                                                    _fp(w, C.c_double)))

    # ---- the reference's public helper members, single-shot on the device
    def clear_ghost_buffer(self):
        self._ck(self.lib.lf_clear_ghost_buffer(self.ctx))

    def draw_ghost(self, channel, r1, r2):
        bbox = (C.c_int * 4)()
        self._ck(self.lib.lf_draw_ghost(self.ctx, int(channel), C.c_float(r1), C.c_float(r2), bbox))
        return tuple(bbox)

    def rasterize_textured_triangle(self, verts12, colour):
        v = np.ascontiguousarray(verts12, np.float32).reshape(12)
        c = np.ascontiguousarray(colour, np.float64).reshape(3)
        bbox = (C.c_int * 4)()
        self._ck(self.lib.lf_rasterize_textured_triangle(self.ctx, _fp(v, C.c_float), _fp(c, C.c_double), bbox))
        return tuple(bbox)

    def fill_textured_pixel(self, verts12, x, y, colour):
        v = np.ascontiguousarray(verts12, np.float32).reshape(12)
        c = np.ascontiguousarray(colour, np.float64).reshape(3)
        self._ck(self.lib.lf_fill_textured_pixel(self.ctx, _fp(v, C.c_float), int(x), int(y), _fp(c, C.c_double)))

    def shift_vertex(self, x, y, scale, shift_amount):
        out = (C.c_double * 2)()
        self._ck(self.lib.lf_shift_vertex(self.ctx, C.c_float(x), C.c_float(y), C.c_float(scale),
                                          C.c_float(shift_amount), out))
        return out[0], out[1]

    def compute_phase(self, flare, u, v):
        out, pos = (C.c_double * 2)(), (C.c_double * 2)()
        self._ck(self.lib.lf_compute_phase(self.ctx, int(flare), C.c_double(u), C.c_double(v), out, pos))
        return complex(out[0], out[1]), (pos[0], pos[1])

    def irradiance_falloff(self, x, y, radius):
        out = (C.c_double * 3)()
        self._ck(self.lib.lf_irradiance_falloff(self.ctx, int(x), int(y), C.c_double(radius), out))
        return np.array(out[:], np.float64)

    def scene_trace_ray(self, origin, direction, min_t=0.0, max_t=float("inf"), seq=0):
        ray = (C.c_double * 8)(*origin, *direction, min_t, max_t)
        out = (C.c_double * 8)()
        self._ck(self.lib.lf_scene_trace_ray(self.ctx, ray, C.c_uint64(seq), out))
        return dict(hit=bool(out[0]), t=out[1], n=np.array(out[2:5]), radiance=np.array(out[5:8]))

    def scene_shade(self, what, origin, direction, t, n, material, min_t=0.0, max_t=float("inf"), seq=0):
        ray = (C.c_double * 8)(*origin, *direction, min_t, max_t)
        nn, mm, out = (C.c_double * 3)(*n), (C.c_double * 4)(*material), (C.c_double * 3)()
        self._ck(self.lib.lf_scene_shade(self.ctx, int(what), ray, C.c_double(t), nn, mm, C.c_uint64(seq), out))
        return np.array(out[:], np.float64)

    def load_lens_file(self, path):
        if not os.path.isabs(path) and not os.path.exists(path):
            path = os.path.join(DATA, path)
        self._ck(self.lib.lf_load_lens_file(self.ctx, path.encode()))

    def set_pupil_target(self, radius_mm=0.0, z_mm=0.0):
        self._ck(self.lib.lf_set_pupil_target(self.ctx, C.c_float(radius_mm), C.c_float(z_mm)))

    def pupil_target(self):
        r, z, zs = C.c_float(), C.c_float(), C.c_float()
        self._ck(self.lib.lf_get_pupil_target(self.ctx, C.byref(r), C.byref(z), C.byref(zs)))
        return dict(radius_mm=r.value, z_mm=z.value, z_sensor_mm=zs.value)

    def aim_at_exit_pupil(self, margin=1.0):
        self._ck(self.lib.lf_aim_at_exit_pupil(self.ctx, C.c_float(margin)))
        return self.pupil_target()

    def set_flare_arithmetic(self, mode=0):
        """0 auto (exact pow in MT19937 parity mode, fast forms with the counter RNG), 1 exact, 2 fast."""
        self._ck(self.lib.lf_set_flare_arithmetic(self.ctx, int(mode)))

    def set_lens_camera(self, mode=1, world_per_mm=0.001, exposure=0.0):
        """The scene term's sample loop images the scene through the prescription (0 = pinhole)."""
        self._ck(self.lib.lf_set_lens_camera(self.ctx, int(mode), C.c_double(world_per_mm), C.c_double(exposure)))

    def set_lens_camera_aim(self, margin=0.0):
        """> 0: the lens camera's samples aim at the exit pupil's image x margin (0: at the march's disc)."""
        self._ck(self.lib.lf_set_lens_camera_aim(self.ctx, C.c_float(margin)))

    def set_lens_camera_surfaces(self, which=LENSCAM_SURFACES_SPHERICAL):
        """LENSCAM_SURFACES_ALL: render_scene_term and lens_camera() accept a lens with aspheric and / or biconic records (the
        scene kernel marches them); LENSCAM_SURFACES_POSED: those, and a lens with pose records (set_lens_poses);
        LENSCAM_SURFACES_SPHERICAL (the default) refuses such lenses as before."""
        if isinstance(which, bool) or not isinstance(which, (int, np.integer)):
            raise ValueError("set_lens_camera_surfaces: LENSCAM_SURFACES_SPHERICAL (0), LENSCAM_SURFACES_ALL (1) or "
                             "LENSCAM_SURFACES_POSED (3)")
        self._ck(self.lib.lf_set_lens_camera_surfaces(self.ctx, int(which)))

    def lens_camera_surfaces(self):
        which = C.c_int(-1)
        self._ck(self.lib.lf_get_lens_camera_surfaces(self.ctx, C.byref(which)))
        return which.value

    def lens_camera_samples(self, pixels):
        """(n_pix, ns_aa, 4) float32 {X, Y, pa, pb}: the sensor point (mm) and the pupil-square coordinates of the lens camera's
        samples 0 .. ns_aa-1 of the listed pixels (p = x + y W), as the device draws them; generate_lens_rays(lam, s[..., 0:2],
        s[..., 2:4]) gives the exit ray and weight the scene kernel carries into the scene for each."""
        pix = np.ascontiguousarray(pixels, np.int32).ravel()
        ns_aa = getattr(self, "_ns_aa", None)     # (what set_params gave the context: the samples per pixel)
        if ns_aa is None or ns_aa < 1:
            raise LensFlareError(4, "lens_camera_samples before set_params (ns_aa samples per pixel)")
        out = np.zeros((len(pix), ns_aa, 4), np.float32)
        self._ck(self.lib.lf_lens_camera_samples(self.ctx, C.c_size_t(len(pix)), _fp(pix, C.c_int), _fp(out, C.c_float)))
        return out

    def lens_camera(self):
        m, w, e, z = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        self._ck(self.lib.lf_get_lens_camera(self.ctx, C.byref(m), C.byref(w), C.byref(e), C.byref(z)))
        return dict(mode=m.value, world_per_mm=w.value, exposure=e.value, entrance_pupil_z_mm=z.value)

    def focus_lens(self, object_distance_mm):
        d = C.c_float()
        self._ck(self.lib.lf_focus_lens(self.ctx, C.c_double(object_distance_mm), C.byref(d)))
        return d.value

    def focus_lens_from_pupil(self, distance_mm):
        """focus_lens with the distance counted from the lens camera's position (the entrance pupil's centre):
        what Camera::focalDistance means"""
        d = C.c_float()
        self._ck(self.lib.lf_focus_lens_from_pupil(self.ctx, C.c_double(distance_mm), C.byref(d)))
        return d.value

    def scene_counters(self):
        v = (C.c_uint64 * 4)()
        self._ck(self.lib.lf_get_scene_counters(self.ctx, v))
        return dict(rays=int(v[0]), isects=int(v[1]), lens_samples=int(v[2]), lens_left=int(v[3]))

    def reset_scene_counters(self):
        self._ck(self.lib.lf_reset_scene_counters(self.ctx))

    def set_ghost_accumulate(self, on):
        self._ck(self.lib.lf_set_ghost_accumulate(self.ctx, int(bool(on))))

    def lens_info(self):
        n, stop, nl, sw, efl = C.c_int(), C.c_int(), C.c_int(), C.c_float(), C.c_double()
        self._ck(self.lib.lf_get_lens_info(self.ctx, C.byref(n), C.byref(stop), C.byref(nl), C.byref(sw), C.byref(efl)))
        return dict(n=n.value, stop=stop.value, n_lambda=nl.value, sensor_width_mm=sw.value, efl_mm=efl.value)

    def native_sqrt(self, x):
        x = np.ascontiguousarray(x, np.float32)
        y = np.empty_like(x)
        self._ck(self.lib.lf_native_sqrt(self.ctx, x.ctypes.data_as(C.POINTER(C.c_float)),
                                         y.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(x.size)))
        return y

    def native_rcp(self, x):
        x = np.ascontiguousarray(x, np.float32)
        y = np.empty_like(x)
        self._ck(self.lib.lf_native_rcp(self.ctx, x.ctypes.data_as(C.POINTER(C.c_float)),
                                        y.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(x.size)))
        return y

    def executed_events(self):
        v = C.c_uint64(0)
        self._ck(self.lib.lf_get_executed_events(self.ctx, C.byref(v)))
        return int(v.value)

    def march_stats(self):
        v = (C.c_uint64 * 4)()
        self._ck(self.lib.lf_get_march_stats(self.ctx, v))
        return dict(executed_events=int(v[0]), remarch_lane_events=int(v[1]), remarch_rows=int(v[2]))

    def reset_counters(self):
        self._ck(self.lib.lf_reset_counters(self.ctx))

    # ---- measurement
    def timing_enable(self, on=True):
        self._ck(self.lib.lf_timing_enable(self.ctx, int(on)))

    def timing_reset(self):
        self._ck(self.lib.lf_timing_reset(self.ctx))

    def timing_get(self, kernel):
        n = C.c_int()
        ms = C.c_double()
        self._ck(self.lib.lf_timing_get(self.ctx, kernel.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value


GROUP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p)


class LensFlareGroup:
    """lf_group_*: one process, n devices (one context + stream per device, one RCCL communicator)."""

    def __init__(self, devices):
        self.lib = load_library()
        self.lib.lf_group_ctx.restype = C.c_void_p
        self.lib.lf_group_last_error.restype = C.c_char_p
        self.g = C.c_void_p()
        dv = (C.c_int * len(devices))(*devices)
        st = self.lib.lf_group_create(C.byref(self.g), len(devices), dv)
        if st != 0:
            self.g = C.c_void_p()
            raise LensFlareError(st, "lf_group_create failed")
        self.ranks = [LensFlare(_borrowed=self.lib.lf_group_ctx(self.g, r)) for r in range(len(devices))]

    def _ck(self, st):
        if st != 0:
            raise LensFlareError(st, self.lib.lf_group_last_error(self.g).decode())

    def set_frame(self, W, H):
        self._ck(self.lib.lf_group_set_frame(self.g, int(W), int(H)))
        for r in self.ranks:
            r.W, r.H = int(W), int(H)

    def for_each(self, fn):
        """fn(LensFlare, rank) on one host thread per device, concurrently."""
        errors = []

        def tramp(ctx, rank, _user):
            try:
                fn(self.ranks[rank], rank)
                return 0
            except LensFlareError as e:
                errors.append(e)
                return e.status
            except Exception as e:  # noqa: BLE001
                errors.append(e)
                return 1
        cb = GROUP_FN(tramp)
        st = self.lib.lf_group_for_each(self.g, cb, None)
        if errors:
            raise errors[0]
        self._ck(st)

    def gather(self, which):
        self._ck(self.lib.lf_group_gather(self.g, int(which)))

    def set_block_deal(self, on=True):
        """the group's frame dealt by 64 x 64-pixel blocks (True) or by tile rows (False, the default)"""
        self._ck(self.lib.lf_group_set_block_deal(self.g, int(bool(on))))

    def share_cull(self, spp):
        """the pre-pass of the next trace_ghosts(spp) shared between the group's devices"""
        self._ck(self.lib.lf_group_share_cull(self.g, int(spp)))

    def close(self):
        if self.g:
            for r in self.ranks:
                r.ctx = C.c_void_p()
            self.lib.lf_group_destroy(self.g)
            self.g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
