"""raytracing-1w_amd -- Python host binding of librt1w.so (the MI355X path tracer).

This is plumbing over the C ABI in ``include/rt1w.h``: every call goes to the
shared library, whose render path is the HIP kernel.  There is no Python or CPU
fallback -- if the library is missing the import fails, and without a GPU
``Context`` raises.

The package name has a hyphen (mandated layout), so import it with::

    import importlib
    rt = importlib.import_module("raytracing-1w_amd")

Method names follow the reference's constructors (src/sphere.rs, src/aarect.rs,
src/material.rs, src/texture.rs, src/bvh.rs, src/camera.rs of hatoo/raytracing-1w).

How an entry is bound: its prototype stands once, in the ``_sig`` table (librt1w.so) or in ``_LAB_SIGS`` (the CPU twins of
librt1w_lab.so); ``_call`` / ``_call_lab`` turn arrays and structs into pointers, make the call and check its code; and an entry
that has a twin has one ``_*_prep`` function that normalises its inputs, checks their shapes and allocates its outputs.
``Context.X`` and ``X_host`` are that preparation handed to ``Context._entry`` or ``_twin``, ``Context.X_device`` is the same
argument list with the caller's addresses in it.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT1W_LIB") or os.path.join(_HERE, "librt1w.so")  # RT1W_LIB: diagnostic builds only

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "librt1w.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C raytracing-1w_amd/csrc` (needs hipcc, gfx950). There is no fallback path."
    )

_lib = C.CDLL(LIB_PATH)
_lab = None

OK = 0
ERR_INVALID, ERR_UNSUPPORTED, ERR_DEVICE, ERR_NOMEM, ERR_STATE, ERR_CANCELLED = -1, -2, -3, -4, -5, -6
ROWS_F64, ROWS_U8 = 0, 1
OUT_SUM = 1
UNSORTED = 2
PROBE_COHERENT = 0x40000000  # measurement only (include/rt1w.h): every wave traces one path 64 times; the frame is not the image
LDS_NODES = 4
GENERIC = 8  # do not use a scene-specialised kernel for this render
OUT_FRAME = 32  # rt1w_render: `out` is the whole image; only the tile's pixels are written, at their image positions
RNG_REFERENCE = 64  # parity mode: the reference's own ChaCha12 stream per pixel (main.rs:964)
NO_NODE_CACHE = 0x10000  # big scenes: the stack-walk kernels without the most visited node records in LDS (rt_walk_table.h)
CLASSIC_WALK = 128  # sphere scenes: the one-entry-per-step walk instead of the pair walk (rt_walk_pair.h)
WAVEFRONT = 16  # big scenes: path state queued in HBM, trace / shade kernels per bounce
SPECIALISE_CACHED_ONLY = 1
SPECIALISE_TILES = 2  # rt1w_context_specialise: load (or compile) the kernel's tile-list form too
TILES_SPECIALISED = 0x40000  # tile entries and the adaptive entries' rounds: the tile-list form of the scene-specialised kernel where a kernel cache has one
AOV_CHANNELS = 8  # rt1w_render_aov: albedo rgb, normal xyz, depth, coverage per pixel
DENOISE_KEEP_ALBEDO = 1  # rt1w_denoise: no albedo demodulation
ADAPTIVE_ONE_LAUNCH = 0x100  # rt1w_adaptive_params.flags: every round is one rt1w_render_tiles launch and one rt1w_accum_merge_tiles

# Context._params: the keywords that are one bit of rt1w_render_params.flags each
_RENDER_FLAGS = {"out_sum": OUT_SUM, "out_frame": OUT_FRAME, "reference_stream": RNG_REFERENCE, "unsorted": UNSORTED, "lds_nodes": LDS_NODES,
                 "generic": GENERIC, "wavefront": WAVEFRONT, "classic_walk": CLASSIC_WALK, "no_node_cache": NO_NODE_CACHE,
                 "probe_coherent": PROBE_COHERENT}


class Rt1wError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rt1w error {code}: {msg}")
        self.code = code


class RenderParams(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "width", "height", "x0", "y0", "tile_w", "tile_h", "spp", "sample_offset",
        "max_depth", "global_seed", "chunk", "flags", "strip_rows", "strip_period", "precision", "partial_mib")]


class SpecialiseInfo(C.Structure):
    _fields_ = [("key", C.c_char * 24), ("active", C.c_uint32), ("from_cache", C.c_uint32), ("compile_ms", C.c_double),
                ("grid", C.c_uint32), ("vgprs", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("segments", C.c_uint64), ("kernel_ms", C.c_double),
                ("total_ms", C.c_double), ("chunk", C.c_uint32), ("n_chunks", C.c_uint32),
                ("grid", C.c_uint32), ("block", C.c_uint32), ("variant", C.c_uint32), ("sorted", C.c_uint32),
                ("passes", C.c_uint32), ("reserved", C.c_uint32)]


class SceneInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_lights", C.c_uint32), ("n_materials", C.c_uint32),
                ("n_textures", C.c_uint32), ("n_perlin", C.c_uint32), ("stack_need", C.c_uint32),
                ("scope_depth", C.c_uint32), ("has_media", C.c_uint32), ("has_textures", C.c_uint32),
                ("has_moving", C.c_uint32), ("variant", C.c_uint32), ("bytes", C.c_uint64)]


_P = C.c_void_p
_D3 = C.c_double * 3


def _sig(name, restype, *argtypes):
    f = getattr(_lib, name)
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


_sig("rt1w_last_error", C.c_char_p)
_sig("rt1w_version", C.c_char_p)
_sig("rt1w_scene_create", C.c_int, C.c_uint64, C.POINTER(_P))
_sig("rt1w_scene_destroy", None, _P)
_sig("rt1w_scene_rng_f64", C.c_int, _P, C.POINTER(C.c_double))
_sig("rt1w_scene_rng_range", C.c_int, _P, C.c_double, C.c_double, C.POINTER(C.c_double))
_sig("rt1w_texture_solid", C.c_int, _P, _D3)
_sig("rt1w_texture_checker", C.c_int, _P, C.c_int, C.c_int)
_sig("rt1w_texture_noise", C.c_int, _P, C.c_double)
_sig("rt1w_texture_noise_tables", C.c_int, _P, C.c_double, _P, _P, _P, _P)
_sig("rt1w_texture_image", C.c_int, _P, _P, C.c_uint32, C.c_uint32)
_sig("rt1w_material_lambertian", C.c_int, _P, C.c_int)
_sig("rt1w_material_metal", C.c_int, _P, _D3, C.c_double)
_sig("rt1w_material_dielectric", C.c_int, _P, C.c_double)
_sig("rt1w_material_diffuse_light", C.c_int, _P, C.c_int)
_sig("rt1w_material_null", C.c_int, _P)
_sig("rt1w_hittable_sphere", C.c_int, _P, _D3, C.c_double, C.c_int)
_sig("rt1w_hittable_moving_sphere", C.c_int, _P, _D3, _D3, C.c_double, C.c_double, C.c_double, C.c_int)
for _n in ("xy", "xz", "yz"):
    _sig(f"rt1w_hittable_{_n}_rect", C.c_int, _P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int)
_sig("rt1w_hittable_aabox", C.c_int, _P, _D3, _D3, C.c_int)
_sig("rt1w_hittable_translate", C.c_int, _P, C.c_int, _D3)
_sig("rt1w_hittable_rotate_y", C.c_int, _P, C.c_int, C.c_double, C.c_double, C.c_double)
_sig("rt1w_hittable_flip_face", C.c_int, _P, C.c_int)
_sig("rt1w_hittable_constant_medium", C.c_int, _P, C.c_int, C.c_double, C.c_int)
_sig("rt1w_hittable_bvh", C.c_int, _P, C.POINTER(C.c_int), C.c_uint32, C.c_double, C.c_double)
_sig("rt1w_scene_set_world", C.c_int, _P, C.c_int)
_sig("rt1w_scene_set_lights", C.c_int, _P, C.POINTER(C.c_int), C.c_uint32)
_sig("rt1w_scene_set_background", C.c_int, _P, _D3)
_sig("rt1w_scene_set_camera", C.c_int, _P, _D3, _D3, _D3, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double)
_sig("rt1w_scene_commit", C.c_int, _P)
_sig("rt1w_scene_build_reference", C.c_int, C.c_int, C.c_uint64, C.c_double, _P, C.c_uint32, C.c_uint32,
     C.POINTER(_P), C.POINTER(C.c_uint32 * 3))
_sig("rt1w_scene_set_walk_order", C.c_int, _P, C.c_uint32)
_sig("rt1w_scene_set_bvh_build", C.c_int, _P, C.c_uint32)
_sig("rt1w_scene_get_bvh_topology", C.c_int64, _P, _P, C.c_uint64)
_sig("rt1w_scene_get_info", C.c_int, _P, C.POINTER(SceneInfo))
_sig("rt1w_scene_copy_flat", C.c_int64, _P, C.c_int, _P, C.c_uint64)
_sig("rt1w_device_count", C.c_int)
_sig("rt1w_context_create", C.c_int, C.c_int, _P, C.POINTER(_P))
_sig("rt1w_context_destroy", None, _P)
_sig("rt1w_context_specialise", C.c_int, _P, C.c_uint32, C.POINTER(SpecialiseInfo))
_sig("rt1w_scene_kernel_key", C.c_int, _P, C.c_char * 24)
_sig("rt1w_scene_kernel_source", C.c_int64, _P, C.c_int, _P, C.c_uint64)
_sig("rt1w_scene_kernel_key_tiles", C.c_int, _P, C.c_char * 24)
_sig("rt1w_scene_kernel_source_tiles", C.c_int64, _P, _P, C.c_uint64)
_sig("rt1w_default_chunk", C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)
_sig("rt1w_scene_default_chunk", C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32)
_sig("rt1w_render", C.c_int, _P, C.POINTER(RenderParams), _P, C.POINTER(Stats))
_sig("rt1w_render_device", C.c_int, _P, C.POINTER(RenderParams), _P, C.POINTER(Stats))
_sig("rt1w_render_u8", C.c_int, _P, C.POINTER(RenderParams), _P, C.POINTER(Stats))
PROGRESS_FN = C.CFUNCTYPE(C.c_int, _P, C.c_uint32, C.c_uint32)
_sig("rt1w_render_rows", C.c_int, _P, C.POINTER(RenderParams), C.c_uint32, C.c_int, _P, PROGRESS_FN, _P, C.POINTER(Stats))
_sig("rt1w_render_aov", C.c_int, _P, C.POINTER(RenderParams), _P, C.POINTER(Stats))
_sig("rt1w_render_aov_device", C.c_int, _P, C.POINTER(RenderParams), _P, C.POINTER(Stats))
_sig("rt1w_render_aov_deep", C.c_int, _P, C.POINTER(RenderParams), C.c_uint32, C.c_double, _P, C.POINTER(Stats))
_sig("rt1w_render_aov_deep_device", C.c_int, _P, C.POINTER(RenderParams), C.c_uint32, C.c_double, _P, C.POINTER(Stats))


class DenoiseParams(C.Structure):
    """rt1w_denoise_params (include/rt1w.h): 0 in iterations or a sigma means the default."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("flags", C.c_uint32),
                ("sigma_colour", C.c_double), ("sigma_normal", C.c_double), ("sigma_depth", C.c_double)]


def _keep(keep_albedo):
    return DENOISE_KEEP_ALBEDO if keep_albedo else 0


def _denoise_params(width, height, iterations=0, keep_albedo=False, sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0, flags=0):
    return DenoiseParams(width, height, iterations, flags | _keep(keep_albedo), sigma_colour, sigma_normal, sigma_depth)


_sig("rt1w_denoise", C.c_int, _P, C.POINTER(DenoiseParams), _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_denoise_device", C.c_int, _P, C.POINTER(DenoiseParams), _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_render_denoised", C.c_int, _P, C.POINTER(RenderParams), C.POINTER(DenoiseParams), _P, C.POINTER(Stats))
_sig("rt1w_render_denoised_deep", C.c_int, _P, C.POINTER(RenderParams), C.POINTER(DenoiseParams), C.c_uint32, C.c_double, _P, C.POINTER(Stats))
_sig("rt1w_batch_variance", C.c_int, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_batch_variance_device", C.c_int, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_denoise_var", C.c_int, _P, C.POINTER(DenoiseParams), _P, _P, _P, C.c_double, _P, C.POINTER(Stats))
_sig("rt1w_denoise_var_device", C.c_int, _P, C.POINTER(DenoiseParams), _P, _P, _P, C.c_double, _P, C.POINTER(Stats))
_sig("rt1w_render_denoised_var", C.c_int, _P, C.POINTER(RenderParams), C.POINTER(DenoiseParams), C.c_uint32, C.c_double, C.c_uint32, C.c_double, _P,
     C.POINTER(Stats))


class AdaptiveParams(C.Structure):
    """rt1w_adaptive_params (include/rt1w.h): `size` is sizeof as this binding lays the struct out; 0 elsewhere means the default."""
    _fields_ = [("size", C.c_uint32), ("tile", C.c_uint32), ("batch_spp", C.c_uint32), ("pilot_batches", C.c_uint32), ("budget_spp", C.c_uint32),
                ("max_spp", C.c_uint32), ("target_error", C.c_double), ("round_share", C.c_double), ("flags", C.c_uint32)]


def adaptive_params(tile=0, batch_spp=0, pilot_batches=0, budget_spp=0, max_spp=0, target_error=0.0, round_share=0.0, keep_albedo=False, flags=0,
                    size=None, one_launch=False):
    return AdaptiveParams(C.sizeof(AdaptiveParams) if size is None else size, tile, batch_spp, pilot_batches, budget_spp, max_spp, target_error,
                          round_share, flags | _keep(keep_albedo) | (ADAPTIVE_ONE_LAUNCH if one_launch else 0))


class Tile(C.Structure):
    """rt1w_tile (include/rt1w.h): one square tile of a list, 16 bytes; reserved = 0."""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("sample_offset", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(Tile) == 16, "rt1w_tile is 16 bytes (include/rt1w.h); it is not one of rt1w_abi_sizeof's"


def _tile_list(tiles):
    """tiles: Tile objects or (x0, y0[, sample_offset[, reserved]]) tuples -> (ctypes array, n)"""
    rec = [t if isinstance(t, Tile) else Tile(*t) for t in tiles]
    return (Tile * max(len(rec), 1))(*rec), len(rec)


_U = C.c_uint32
_sig("rt1w_accum_merge", C.c_int, _P, _U, _U, _U, _U, _U, _U, _U, _U, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_accum_merge_device", C.c_int, _P, _U, _U, _U, _U, _U, _U, _U, _U, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_accum_merge_tiles", C.c_int, _P, _U, _U, _U, _P, _U, _U, _U, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_accum_merge_tiles_device", C.c_int, _P, _U, _U, _U, _P, _U, _U, _U, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_render_tiles", C.c_int, _P, C.POINTER(RenderParams), _U, _P, _U, _P, C.POINTER(Stats))
_sig("rt1w_render_tiles_device", C.c_int, _P, C.POINTER(RenderParams), _U, _P, _U, _P, C.POINTER(Stats))
_sig("rt1w_accum_resolve", C.c_int, _P, _U, _U, _U, _P, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_accum_resolve_device", C.c_int, _P, _U, _U, _U, _P, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_accum_tile_error", C.c_int, _P, _U, _U, _U, _P, _P, C.POINTER(Stats))
_sig("rt1w_accum_tile_error_device", C.c_int, _P, _U, _U, _U, _P, _P, C.POINTER(Stats))
_sig("rt1w_adaptive_select", C.c_int, C.POINTER(AdaptiveParams), _U, _U, _U, _U, _P, _P, _P, _U)
_sig("rt1w_render_adaptive", C.c_int, _P, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), C.POINTER(DenoiseParams), C.c_double, _P, _P,
     C.POINTER(Stats))
_sig("rt1w_halves_resolve", C.c_int, _P, _U, _U, _U, _P, _P, _P, _P, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_halves_resolve_device", C.c_int, _P, _U, _U, _U, _P, _P, _P, _P, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_denoise_var_halves", C.c_int, _P, C.POINTER(DenoiseParams), _P, _P, _P, _P, _P, C.c_double, _P, _P, C.POINTER(Stats))
_sig("rt1w_denoise_var_halves_device", C.c_int, _P, C.POINTER(DenoiseParams), _P, _P, _P, _P, _P, C.c_double, _P, _P, C.POINTER(Stats))
_sig("rt1w_tile_error_map", C.c_int, _P, _U, _U, _U, _P, _P, C.POINTER(Stats))
_sig("rt1w_tile_error_map_device", C.c_int, _P, _U, _U, _U, _P, _P, C.POINTER(Stats))
_sig("rt1w_render_adaptive_filtered", C.c_int, _P, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), C.POINTER(DenoiseParams), C.c_double, _P, _P,
     _P, C.POINTER(Stats))
_sig("rt1w_denoise_cross", C.c_int, _P, C.POINTER(DenoiseParams), _P, _P, _P, _P, _P, C.c_double, _P, _P, C.POINTER(Stats))
_sig("rt1w_denoise_cross_device", C.c_int, _P, C.POINTER(DenoiseParams), _P, _P, _P, _P, _P, C.c_double, _P, _P, C.POINTER(Stats))
_sig("rt1w_render_adaptive_cross", C.c_int, _P, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), C.POINTER(DenoiseParams), C.c_double, _P, _P,
     _P, C.POINTER(Stats))
_sig("rt1w_render_aov_tiles", C.c_int, _P, C.POINTER(RenderParams), _U, _P, _U, _P, C.POINTER(Stats))
_sig("rt1w_render_aov_tiles_device", C.c_int, _P, C.POINTER(RenderParams), _U, _P, _U, _P, C.POINTER(Stats))
_sig("rt1w_guides_merge_tiles", C.c_int, _P, _U, _U, _U, _P, _U, _U, _P, _P, C.POINTER(Stats))
_sig("rt1w_guides_merge_tiles_device", C.c_int, _P, _U, _U, _U, _P, _U, _U, _P, _P, C.POINTER(Stats))
_sig("rt1w_guides_resolve", C.c_int, _P, _U, _U, _P, _P, C.POINTER(Stats))
_sig("rt1w_guides_resolve_device", C.c_int, _P, _U, _U, _P, _P, C.POINTER(Stats))
_sig("rt1w_render_adaptive_guided", C.c_int, _P, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), C.POINTER(DenoiseParams), C.c_double, _P, _P,
     _P, C.POINTER(Stats))


class Camera(C.Structure):
    """rt1w_camera: the ten quantities of camera.rs:7-18 as the kernels take them."""
    _fields_ = [(n, _D3) for n in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w")] + \
               [(n, C.c_double) for n in ("lens_radius", "time0", "time1")]

    def array(self):
        """The 24 doubles, in the struct's order."""
        return np.frombuffer(bytes(self), dtype=np.float64).copy()

    @classmethod
    def of(cls, cam):
        """A Camera from a Camera or from 24 doubles."""
        return cam if isinstance(cam, cls) else cls.from_buffer_copy(np.ascontiguousarray(cam, dtype=np.float64).reshape(24).tobytes())


class TemporalParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("max_history", C.c_uint32),
                ("depth_tol", C.c_double), ("normal_min", C.c_double)]


assert C.sizeof(TemporalParams) == 32, "rt1w_temporal_params is 32 bytes (include/rt1w.h); it is not one of rt1w_abi_sizeof's"


def _temporal_params(width, height, keep_albedo=False, max_history=0, depth_tol=0.0, normal_min=0.0, flags=0):
    return TemporalParams(width, height, flags | _keep(keep_albedo), max_history, depth_tol, normal_min)


class HitParams(C.Structure):
    """rt1w_hit_params: n rays; ray r draws from the stream of pixel seed first_stream + r, sample `sample`, `global_seed`."""
    _fields_ = [("n", C.c_uint64), ("first_stream", C.c_uint64), ("global_seed", C.c_uint64), ("sample", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(HitParams) == 32, "rt1w_hit_params is 32 bytes (include/rt1w.h); it is not one of rt1w_abi_sizeof's"
HIT_RAY = 9  # rt1w_hit: origin xyz, direction xyz, time, t_min, t_max per ray
HIT_RECORD = 12  # rt1w_hit: hit, t, p xyz, normal xyz, u, v, front_face, material id per ray
HIT_NO_NODE = 0xFFFFFFFF  # the node index of a miss
_sig("rt1w_hit", C.c_int, _P, C.POINTER(HitParams), _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_hit_device", C.c_int, _P, C.POINTER(HitParams), _P, _P, _P, C.POINTER(Stats))


class RayColorParams(C.Structure):
    """rt1w_ray_color_params: n rays, spp samples each; sample k of ray r draws from the stream of pixel seed first_stream + r, sample
    sample_offset + k, `global_seed`."""
    _fields_ = [("n", C.c_uint64), ("first_stream", C.c_uint64), ("global_seed", C.c_uint64), ("spp", C.c_uint32), ("sample_offset", C.c_uint32),
                ("max_depth", C.c_uint32), ("chunk", C.c_uint32), ("stride", C.c_uint32), ("flags", C.c_uint32), ("partial_mib", C.c_uint32),
                ("reserved", C.c_uint32)]


RAY_RECORD = 7  # rt1w_ray_color: origin xyz, direction xyz, time per ray; a record may be longer (its stride)
_sig("rt1w_ray_color", C.c_int, _P, C.POINTER(RayColorParams), _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_ray_color_device", C.c_int, _P, C.POINTER(RayColorParams), _P, _P, _P, C.POINTER(Stats))


class PathParams(C.Structure):
    """rt1w_path_params: n states advanced by up to `steps` levels of ray_color each; the streams take `global_seed`."""
    _fields_ = [("n", C.c_uint64), ("global_seed", C.c_uint64), ("steps", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


# rt1w_path_state, 128 bytes: the next ray, the path's throughput and radiance so far, its Philox stream and position, the depth left, status
PATH_STATE = np.dtype([("ray", "<f8", (7,)), ("beta", "<f8", (3,)), ("radiance", "<f8", (3,)), ("stream", "<u8"), ("sample", "<u4"), ("word", "<u4"),
                       ("depth_left", "<u4"), ("status", "<u4")])
PATH_ALIVE, PATH_TRACED = 1, 2  # RT1W_PATH_ALIVE, RT1W_PATH_TRACED; the event of the last level: (status >> 8) & 0xFF, a key of PATH_EVENTS
PATH_EVENTS = {0: "none", 1: "miss", 2: "depth", 3: "light", 4: "absorbed", 5: "lambertian", 6: "metal", 7: "dielectric", 8: "isotropic", 9: "untraced"}
PATH_NO_NODE = 0xFFFFFFFF  # out_node of a miss, a level without depth, a dead state, a ray that is not traced
_sig("rt1w_path_step", C.c_int, _P, C.POINTER(PathParams), _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_path_step_device", C.c_int, _P, C.POINTER(PathParams), _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_path_begin", C.c_int, _P, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _P, C.c_uint64, _P, C.POINTER(Stats))
_sig("rt1w_path_begin_device", C.c_int, _P, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _P, C.c_uint64, _P, C.POINTER(Stats))

_CAM_ARGS = [_D3, _D3, _D3] + [C.c_double] * 6
_sig("rt1w_reference_camera", C.c_int, C.c_int, _D3, _D3, _D3, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
_sig("rt1w_context_set_camera", C.c_int, _P, *_CAM_ARGS)
_sig("rt1w_context_get_camera", C.c_int, _P, C.POINTER(Camera))
_sig("rt1w_temporal_accumulate", C.c_int, _P, C.POINTER(TemporalParams), _P, _P, C.POINTER(Camera), _P, _P, _P, C.POINTER(Camera), _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_temporal_accumulate_device", C.c_int, _P, C.POINTER(TemporalParams), _P, _P, C.POINTER(Camera), _P, _P, _P, C.POINTER(Camera), _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_render_temporal", C.c_int, _P, C.POINTER(RenderParams), C.POINTER(TemporalParams), C.POINTER(DenoiseParams), _P, C.POINTER(Stats))
_sig("rt1w_temporal_reset", C.c_int, _P)
_sig("rt1w_temporal_moments", C.c_int, _P, C.POINTER(TemporalParams), _P, _P, C.POINTER(Camera), _P, _P, _P, _P, C.POINTER(Camera), _P, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_temporal_moments_device", C.c_int, _P, C.POINTER(TemporalParams), _P, _P, C.POINTER(Camera), _P, _P, _P, _P, C.POINTER(Camera), _P, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_temporal_variance", C.c_int, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_temporal_variance_device", C.c_int, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, C.POINTER(Stats))
_sig("rt1w_render_temporal_var", C.c_int, _P, C.POINTER(RenderParams), C.POINTER(TemporalParams), C.POINTER(DenoiseParams), C.c_double, _P, C.POINTER(Stats))
_sig("rt1w_abi_sizeof", C.c_uint32, C.c_int)
_sig("rt1w_host_alloc", C.c_int, C.c_uint64, C.POINTER(_P))
_sig("rt1w_host_free", C.c_int, _P)
_sig("rt1w_host_register", C.c_int, _P, C.c_uint64)
_sig("rt1w_host_unregister", C.c_int, _P)
_sig("rt1w_resolve", C.c_int, _P, C.c_uint64, C.c_uint32, _P)
_sig("rt1w_quantize", C.c_int, _P, C.c_uint64, _P)
_sig("rt1w_format_ppm", C.c_int64, _P, C.c_uint32, C.c_uint32, _P, C.c_uint64)
_sig("rt1w_debug_eval", C.c_int, _P, C.c_int, _P, _P, _P, C.c_uint64)
_sig("rt1w_debug_aabb", C.c_int, _P, _P, _P, _P, C.c_uint64)
_sig("rt1w_debug_stamps", C.c_int, _P, C.POINTER(C.c_uint64 * 16), C.c_int)
_sig("rt1w_debug_texture", C.c_int, _P, C.c_int, C.c_uint32, _P, _P, C.c_uint64)


for _i, _t in enumerate((RenderParams, Stats, SceneInfo, SpecialiseInfo)):
    if _lib.rt1w_abi_sizeof(_i) != C.sizeof(_t):
        raise ImportError(f"librt1w.so and this binding disagree on the layout of {_t.__name__}: rebuild the library")
if _lib.rt1w_abi_sizeof(6) != C.sizeof(Camera):
    raise ImportError("librt1w.so and this binding disagree on the layout of Camera: rebuild the library")
if _lib.rt1w_abi_sizeof(8) != C.sizeof(RayColorParams) or C.sizeof(RayColorParams) != 56:
    raise ImportError("librt1w.so and this binding disagree on the layout of RayColorParams: rebuild the library")
if _lib.rt1w_abi_sizeof(11) != PATH_STATE.itemsize or PATH_STATE.itemsize != 128 or _lib.rt1w_abi_sizeof(10) != C.sizeof(PathParams):
    raise ImportError("librt1w.so and this binding disagree on the layout of PATH_STATE or PathParams: rebuild the library")


# The functions of librt1w_lab.so this binding calls (csrc/walk_lab.h), name -> argtypes; every one returns int.  load_lab applies it.
_I, _F, _N = C.c_int, C.c_double, C.c_uint64
_PR, _PD, _PT, _PC = C.POINTER(RenderParams), C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.POINTER(Camera)
_LAB_SIGS = {
    "rt1w_lab_aov_host": [_P, _PR, _P],
    "rt1w_lab_aov_deep_host": [_P, _PR, _U, _F, _P, C.POINTER(_N), _P],
    "rt1w_lab_aov_tiles_host": [_P, _PR, _U, _P, _U, _P],
    "rt1w_lab_hit_host": [_P, C.POINTER(HitParams), _P, _P, _P],
    "rt1w_lab_texture_host": [_P, _I, _U, _P, _P, _N],
    "rt1w_lab_camera_rays_host": [_P, _PR, _P],
    "rt1w_lab_camera_rays_pos_host": [_P, _PR, _P, _P],
    "rt1w_lab_ray_color_host": [_P, C.POINTER(RayColorParams), _P, _P, _P, C.POINTER(_N)],
    "rt1w_lab_ray_color_counts_host": [_P, C.POINTER(RayColorParams), _P, _P, _P, C.POINTER(_N), _P],
    "rt1w_lab_path_step_host": [_P, C.POINTER(PathParams), _P, _P, _P, C.POINTER(_N)],
    "rt1w_lab_path_begin_host": [_P, _U, _U, _N, _U, _P, _N, _P],
    "rt1w_lab_denoise_host": [_PD, _P, _P, _P],
    "rt1w_lab_batch_variance_host": [_U] * 5 + [_P] * 4,
    "rt1w_lab_denoise_var_host": [_PD, _P, _P, _P, _F, _P],
    "rt1w_lab_accum_merge_host": [_U] * 8 + [_P] * 3,
    "rt1w_lab_accum_merge_tiles_host": [_U] * 3 + [_P] + [_U] * 3 + [_P] * 3,
    "rt1w_lab_accum_resolve_host": [_U] * 3 + [_P] * 4,
    "rt1w_lab_tile_error_host": [_U] * 3 + [_P] * 2,
    "rt1w_lab_halves_resolve_host": [_U] * 3 + [_P] * 7,
    "rt1w_lab_denoise_var_halves_host": [_PD] + [_P] * 5 + [_F] + [_P] * 4,
    "rt1w_lab_tile_error_map_host": [_U] * 3 + [_P] * 2,
    "rt1w_lab_denoise_cross_host": [_PD] + [_P] * 5 + [_F] + [_P] * 3,
    "rt1w_lab_guides_merge_tiles_host": [_U] * 3 + [_P] + [_U] * 2 + [_P] * 2,
    "rt1w_lab_guides_resolve_host": [_U] * 2 + [_P] * 2,
    "rt1w_lab_temporal_host": [_PT, _P, _P, _PC, _P, _P, _P, _PC, _P, _P, _P, _P],
    "rt1w_lab_temporal_moments_host": [_PT, _P, _P, _PC, _P, _P, _P, _P, _PC, _P, _P, _P, _P, _P],
    "rt1w_lab_temporal_variance_host": [_U] * 2 + [_P] * 5,
    "rt1w_lab_scene_set_camera": [_P] + _CAM_ARGS,
    "rt1w_lab_scene_get_camera": [_P, _PC],
    "rt1w_lab_denoise_elementary": [_I, _I, _P, _P, _N, _P],
    "rt1w_lab_f32_exact": [_I],
    "rt1w_lab_f32_elementary": [_I, _I, _P, _P, _N, _P],
    "rt1w_lab_f32_draws": [_I, _I, _P, C.c_float, C.c_float, _N, _P],
}


def load_lab():
    """Load the diagnostics library librt1w_lab.so (the trace-only harness and the wavefront form: measured opt-ins that are not in the
    product library).  Loading it registers the wavefront form with librt1w.so; RT1W_WAVEFRONT renders need it."""
    global _lab
    if _lab is None:
        lab = C.CDLL(os.path.join(os.path.dirname(LIB_PATH), "librt1w_lab.so"))
        for name, argtypes in _LAB_SIGS.items():
            fn = getattr(lab, name)
            fn.restype = C.c_int
            fn.argtypes = argtypes
        _lab = lab
    return _lab


def last_error():
    return _lib.rt1w_last_error().decode()


def version():
    return _lib.rt1w_version().decode()


def _ck(rc):
    if rc < 0:
        raise Rt1wError(rc, last_error())
    return rc


def _ck_lab(rc, name):
    """Most twins do not set rt1w_last_error: the error names the function."""
    if rc < 0:
        raise Rt1wError(rc, name)
    return rc


def _stats_dict(st):
    return {n: getattr(st, n) for n, _ in Stats._fields_}


def _c_args(args):
    """Arguments as a C function takes them: an ndarray is its data pointer, a Structure a reference to it; None, numbers (device
    addresses among them), handles and ctypes arrays pass as they are.  The pointers are explicit, so the call is valid under the
    prototypes of the tables and under all-void* ones."""
    return [a.ctypes.data_as(_P) if isinstance(a, np.ndarray) else C.byref(a) if isinstance(a, C.Structure) else a for a in args]


def _call(fn, *args, stats=True):
    """One call of librt1w.so, checked.  stats: `fn` takes an rt1w_stats* last; it is appended and comes back as a dict.  Else the
    function's (non-negative) return value."""
    if not stats:
        return _ck(fn(*_c_args(args)))
    st = Stats()
    _ck(fn(*_c_args(args), C.byref(st)))
    return _stats_dict(st)


def _call_lab(name, *args, says_why=False):
    """One call of librt1w_lab.so's function `name`, checked.  says_why: the function sets rt1w_last_error when it refuses."""
    rc = getattr(load_lab(), name)(*_c_args(args))
    return _ck(rc) if says_why else _ck_lab(rc, name)


def _twin(name, prep, *extra, says_why=False):
    """A CPU twin: `prep` = (arguments, results) of the entry's _*_prep, `extra` the twin's optional outputs.  Returns the results."""
    args, out = prep
    _call_lab(name, *args, *extra, says_why=says_why)
    return out


def _ret(out, stats, with_stats):
    """`out` (an array or a tuple of arrays), with the stats dict after it if asked for"""
    if not with_stats:
        return out
    return out + (stats,) if isinstance(out, tuple) else (out, stats)


def _f64(*arrays):
    return [np.ascontiguousarray(x, dtype=np.float64) for x in arrays]


def _frame_and_aov(frame, aov):
    f, a = _f64(frame, aov)
    if f.ndim != 3 or f.shape[2] != 3 or a.shape != f.shape[:2] + (AOV_CHANNELS,):
        raise ValueError("frame must be [h, w, 3] and aov [h, w, 8]")
    return f, a


def _variance_of(var, frame):
    v, = _f64(var)
    if v.shape != frame.shape[:2]:
        raise ValueError("var must be [h, w]")
    return v


ACCUM_RECORD = 8  # rt1w_accum_*: S rgb, m, mean_d, M2_d, mean_p, M2_p per pixel
ACCUM_NO_ESTIMATE = -1.0


def _accum_of(acc):
    a, = _f64(acc)
    if a.ndim != 3 or a.shape[2] != ACCUM_RECORD:
        raise ValueError("acc must be [h, w, 8]")
    return a


GUIDES_RECORD = 9  # rt1w_guides_*: the 8 first-hit feature sums and N, the samples merged, per pixel


def _guides_of(gacc):
    g, = _f64(gacc)
    if g.ndim != 3 or g.shape[2] != GUIDES_RECORD:
        raise ValueError("gacc must be [h, w, 9]")
    return g


def _error_map_of(err_px):
    e, = _f64(err_px)
    if e.ndim != 2:
        raise ValueError("err_px must be [h, w]")
    return e


# The preparation of every entry that has a CPU twin, written once for Context.X and X_host: inputs as contiguous float64, their shapes
# checked, the outputs allocated.  Each returns (the C arguments after the context and before the stats, what the entry returns).

def _aov_prep(deep, width, height, spp, tile, sample_offset, global_seed, variant, strips):
    """deep: () for the first-hit entries, (max_specular, max_fuzz) for the deep ones"""
    p = Context._params(width, height, spp, 0, tile, sample_offset, global_seed, 0, False, variant=variant, strips=strips)
    out = np.empty((p.tile_h, p.tile_w, AOV_CHANNELS), dtype=np.float64)
    return (p, *deep, out), out


def _aov_tiles_prep(width, height, spp, tile, tiles, sample_offset, global_seed, variant, flags, strips, f32):
    p = Context._params(width, height, spp, 0, None, sample_offset, global_seed, 0, False, variant=variant, strips=strips, f32=f32, flags=flags)
    rec, n = _tile_list(tiles)
    out = np.empty((n, tile, tile, AOV_CHANNELS), dtype=np.float64)
    return (p, tile, rec, n, out), out


def _hit_params(n, first_stream=0, sample=0, global_seed=0, variant=None, flags=0):
    return HitParams(n, first_stream, global_seed, sample, flags | (0 if variant is None else (variant + 1) << 8))


def _hit_prep(rays, t_min, t_max, first_stream, sample, global_seed, variant):
    """rays [n, 9], or [n, 7] = origin, direction, time with t_min and t_max filled in for every ray"""
    r, = _f64(rays)
    if r.ndim != 2 or r.shape[1] not in (7, HIT_RAY):
        raise ValueError("rays must be [n, 7] (origin, direction, time) or [n, 9] (+ t_min, t_max)")
    if r.shape[1] == 7:
        r = np.concatenate([r, np.full((r.shape[0], 1), t_min, dtype=np.float64), np.full((r.shape[0], 1), t_max, dtype=np.float64)], axis=1)
    out = np.empty((r.shape[0], HIT_RECORD), dtype=np.float64)
    node = np.empty(r.shape[0], dtype=np.uint32)
    return (_hit_params(r.shape[0], first_stream, sample, global_seed, variant), r, out, node), (out, node)


def _ray_color_params(n, spp=1, sample_offset=0, max_depth=50, first_stream=0, global_seed=0, chunk=0, stride=0, out_sum=False, generic=False,
                      partial_mib=0, flags=0, f32=False):
    if f32:  # the parameter block has no precision member: the refusal include/rt1w.h states for single precision is the binding's
        raise Rt1wError(ERR_UNSUPPORTED, "ray_color: the ray-list kernels are f64 only")
    flags |= (_RENDER_FLAGS["out_sum"] if out_sum else 0) | (_RENDER_FLAGS["generic"] if generic else 0)
    return RayColorParams(n, first_stream, global_seed, spp, sample_offset, max_depth, chunk, stride, flags, int(partial_mib), 0)


def _ray_color_prep(rays, start_word, kw):
    """rays [n, stride >= 7] = origin, direction, time, .. (the record's other doubles are not read); start_word None or uint32 [n]"""
    r, = _f64(rays)
    if r.ndim != 2 or r.shape[1] < RAY_RECORD:
        raise ValueError("rays must be [n, 7] (origin, direction, time) or wider ([n, 9]: rt1w_hit's records)")
    sw = None if start_word is None else np.ascontiguousarray(start_word, dtype=np.uint32)
    if sw is not None and sw.shape != (r.shape[0],):
        raise ValueError("start_word must be [n]")
    out = np.empty((r.shape[0], 3), dtype=np.float64)
    return (_ray_color_params(r.shape[0], stride=r.shape[1], **kw), r, sw, out), out


def _path_params(n, steps=1, global_seed=0, variant=None, flags=0):
    return PathParams(n, global_seed, steps, flags | (0 if variant is None else (variant + 1) << 8), (C.c_uint32 * 2)(0, 0))


def _path_states(states):
    """states: a PATH_STATE array [n], or float64 [n, 16] holding the same 128 bytes per row"""
    s = np.asarray(states)
    if s.dtype != PATH_STATE:
        if s.dtype != np.float64 or s.ndim != 2 or s.shape[1] != 16:
            raise ValueError("states must be a PATH_STATE array [n] or float64 [n, 16]")
        s = np.ascontiguousarray(s).view(PATH_STATE)
    return np.ascontiguousarray(s).reshape(-1)


def _path_step_prep(states, steps, global_seed, variant):
    s = _path_states(states)
    out = np.empty_like(s)
    node = np.empty(s.shape[0], dtype=np.uint32)
    return (_path_params(s.shape[0], steps, global_seed, variant), s, out, node), (out, node)


def _path_begin_prep(width, height, pixels, global_seed, max_depth):
    """pixels [n, 3] = i, j, sample"""
    px = np.ascontiguousarray(pixels, dtype=np.uint32)
    if px.ndim != 2 or px.shape[1] != 3:
        raise ValueError("pixels must be [n, 3] (i, j, sample)")
    out = np.empty(px.shape[0], dtype=PATH_STATE)
    return (width, height, global_seed, max_depth, px, px.shape[0], out), out


def _path_tensor(t, what):
    """a torch tensor of path states on a GPU, [n, 16] float64 contiguous: (its address, n).  The entries run on the context's own
    stream, so what torch has enqueued for the tensor's device -- the gather that compacted the list, say -- is waited for here"""
    if t.dim() != 2 or t.shape[1] != 16 or str(t.dtype) != "torch.float64" or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"{what} must be a contiguous float64 tensor [n, 16] on the GPU")
    import torch
    torch.cuda.current_stream(t.device).synchronize()
    return t.data_ptr(), t.shape[0]


def _denoise_prep(frame, aov, kw):
    f, a = _frame_and_aov(frame, aov)
    out = np.empty_like(f)
    return (_denoise_params(f.shape[1], f.shape[0], **kw), f, a, out), out


def _batch_variance_prep(sums, aov, batch_spp, keep_albedo):
    s, a = _f64(sums, aov)
    if s.ndim != 4 or s.shape[3] != 3 or a.shape != s.shape[1:3] + (AOV_CHANNELS,):
        raise ValueError("sums must be [batches, h, w, 3] and aov [h, w, 8]")
    frame, var = np.empty(s.shape[1:], dtype=np.float64), np.empty(s.shape[1:3], dtype=np.float64)
    return (s.shape[2], s.shape[1], s.shape[0], batch_spp, _keep(keep_albedo), s, a, frame, var), (frame, var)


def _denoise_var_prep(frame, aov, var, sigma_variance, kw):
    f, a = _frame_and_aov(frame, aov)
    v = _variance_of(var, f)
    out = np.empty_like(f)
    return (_denoise_params(f.shape[1], f.shape[0], **kw), f, a, v, sigma_variance, out), out


def _halves_filter_prep(frame, aov, var, half_a, half_b, sigma_variance, kw):
    """denoise_var_halves and denoise_cross"""
    f, a = _frame_and_aov(frame, aov)
    v = _variance_of(var, f)
    ha, hb = _f64(half_a, half_b)
    if ha.shape != f.shape or hb.shape != f.shape:
        raise ValueError("half_a and half_b must be [h, w, 3] like the frame")
    out, err = np.empty_like(f), np.empty(f.shape[:2])
    return (_denoise_params(f.shape[1], f.shape[0], **kw), f, a, v, ha, hb, sigma_variance, out, err), (out, err)


def _merge_prep(acc, tile_sums, aov, batch_spp, x0, y0, keep_albedo):
    a = _accum_of(acc).copy()
    s, g = _f64(tile_sums, aov)
    if s.ndim != 3 or s.shape[2] != 3 or g.shape != a.shape[:2] + (AOV_CHANNELS,):
        raise ValueError("tile_sums must be [tile_h, tile_w, 3] and aov [h, w, 8]")
    return (a.shape[1], a.shape[0], x0, y0, s.shape[1], s.shape[0], batch_spp, _keep(keep_albedo), s, g, a), a


def _merge_tiles_prep(acc, tile_sums, aov, batch_spp, tile, tiles, keep_albedo):
    """An empty list skips the shape check, as in _guides_merge_prep: the library's own refusal is what the caller sees."""
    a = _accum_of(acc).copy()
    s, g = _f64(tile_sums, aov)
    rec, n = _tile_list(tiles)
    if n and (s.shape != (n, tile, tile, 3) or g.shape != a.shape[:2] + (AOV_CHANNELS,)):
        raise ValueError("tile_sums must be [n_tiles, tile, tile, 3] and aov [h, w, 8]")
    return (a.shape[1], a.shape[0], tile, rec, n, batch_spp, _keep(keep_albedo), s, g, a), a


def _accum_resolve_prep(acc, batch_spp):
    a = _accum_of(acc)
    hw = a.shape[:2]
    out = np.empty(hw + (3,)), np.empty(hw), np.empty(hw)
    return (a.shape[1], a.shape[0], batch_spp, a, *out), out


def _halves_resolve_prep(acc_a, acc_b, batch_spp):
    a, b = _accum_of(acc_a), _accum_of(acc_b)
    if a.shape != b.shape:
        raise ValueError("acc_a and acc_b must have one shape")
    hw = a.shape[:2]
    out = np.empty(hw + (3,)), np.empty(hw), np.empty(hw + (3,)), np.empty(hw + (3,)), np.empty(hw)
    return (a.shape[1], a.shape[0], batch_spp, a, b, *out), out


def _tile_error_prep(px, tile):
    """accum_tile_error (px = _accum_of(acc)) and tile_error_map (px = _error_map_of(err_px)).  The output is sized for a tile of at
    least 1; the library is handed `tile` itself and refuses 0."""
    h, w = px.shape[:2]
    t = max(int(tile), 1)
    err = np.empty(((h + t - 1) // t, (w + t - 1) // t))
    return (w, h, tile, px, err), err


def _guides_merge_prep(gacc, tile_sums, spp, tile, tiles):
    g = _guides_of(gacc).copy()
    s, = _f64(tile_sums)
    rec, n = _tile_list(tiles)
    if n and s.shape != (n, tile, tile, AOV_CHANNELS):
        raise ValueError("tile_sums must be [n_tiles, tile, tile, 8]")
    return (g.shape[1], g.shape[0], tile, rec, n, spp, s, g), g


def _guides_resolve_prep(gacc):
    g = _guides_of(gacc)
    aov = np.empty(g.shape[:2] + (AOV_CHANNELS,))
    return (g.shape[1], g.shape[0], g, aov), aov


def _temporal_prep(cur_frame, cur_aov, cur_cam, prev_hist, prev_m2, prev_len, prev_aov, prev_cam, kw):
    """temporal_accumulate (prev_m2 None) and temporal_moments: the second-moment channel goes in after prev_hist and comes back after hist"""
    f, a = _frame_and_aov(cur_frame, cur_aov)
    h, q = _frame_and_aov(prev_hist, prev_aov)
    n, = _f64(prev_len)
    if h.shape != f.shape or n.shape != f.shape[:2]:
        raise ValueError("prev_hist must be [h, w, 3] and prev_len [h, w], the current frame's size")
    m = () if prev_m2 is None else tuple(_f64(prev_m2))
    if m and m[0].shape != f.shape[:2]:
        raise ValueError("prev_m2 must be [h, w], the current frame's size")
    p = _temporal_params(f.shape[1], f.shape[0], **kw)
    out = (np.empty_like(f),) + tuple(np.empty_like(n) for _ in m) + (np.empty_like(n), np.empty_like(f))
    return (p, f, a, Camera.of(cur_cam), h, *m, n, q, Camera.of(prev_cam), *out), out


def _temporal_variance_prep(hist, m2, length, aov):
    h, a = _frame_and_aov(hist, aov)
    m, n = _f64(m2, length)
    if m.shape != h.shape[:2] or n.shape != h.shape[:2]:
        raise ValueError("m2 and len must be [h, w], the history's size")
    var = np.empty_like(m)
    return (h.shape[1], h.shape[0], h, m, n, a, var), var


def reference_camera(arm, aspect_ratio=None):
    """The arguments Scene.reference(arm) hands to set_camera (rt1w_reference_camera), as a dict of Scene.set_camera's /
    Context.set_camera's keywords."""
    lf, la, up = _D3(), _D3(), _D3()
    vfov, ap, fd = C.c_double(), C.c_double(), C.c_double()
    _ck(_lib.rt1w_reference_camera(arm, lf, la, up, C.byref(vfov), C.byref(ap), C.byref(fd)))
    if aspect_ratio is None:
        aspect_ratio = 1.0 if (arm in (5, 6) or arm < 0 or arm > 6) else 16.0 / 9.0
    return {"look_from": tuple(lf), "look_at": tuple(la), "vup": tuple(up), "vfov_deg": vfov.value, "aspect_ratio": aspect_ratio,
            "aperture": ap.value, "focus_dist": fd.value, "time0": 0.0, "time1": 1.0}


def orbit_camera(args, degrees):
    """`args` (a dict as reference_camera's) with look_from turned about the vertical axis through look_at by `degrees`: the
    turntable of the CLI's --orbit."""
    import math
    lf, la = args["look_from"], args["look_at"]
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    dx, dz = lf[0] - la[0], lf[2] - la[2]
    return dict(args, look_from=(la[0] + c * dx + s * dz, lf[1], la[2] - s * dx + c * dz))


def _v3(v):
    return _D3(float(v[0]), float(v[1]), float(v[2]))


def device_count():
    return _lib.rt1w_device_count()


def default_chunk(tile_w, tile_h, spp):
    return _lib.rt1w_default_chunk(tile_w, tile_h, spp)


_EARTH = None


def earth_rgb8():
    """Decoded 1024x512 RGB8 earth map used by scene arms 3 and 7 (host one-shot).

    The reference decodes assets/earthmap.jpg with the `image` crate (src/main.rs:347-348);
    here PIL decodes the same asset; decoders may differ by 1 LSB per texel (unpinned).
    """
    global _EARTH
    if _EARTH is None:
        from PIL import Image
        im = Image.open(os.path.join(_HERE, "assets", "earthmap.jpg")).convert("RGB")
        _EARTH = np.ascontiguousarray(np.asarray(im, dtype=np.uint8))
    return _EARTH


class Scene:
    """Scene under construction / committed (rt1w_scene)."""

    def __init__(self, build_seed=1, _handle=None, _defaults=None):
        if _handle is None:
            h = _P()
            _ck(_lib.rt1w_scene_create(C.c_uint64(build_seed), C.byref(h)))
            _handle = h
        self._h = _handle
        self.defaults = _defaults  # (image_width, image_height, samples_per_pixel) of a reference arm
        self._keep = []

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.rt1w_scene_destroy(self._h)
            self._h = None

    @classmethod
    def reference(cls, arm, build_seed=1, aspect_ratio=None):
        """The scene table of the reference's main (src/main.rs:815-937)."""
        if aspect_ratio is None:
            aspect_ratio = 1.0 if (arm in (5, 6) or arm < 0 or arm > 6) else 16.0 / 9.0
        earth = None
        ew = eh = 0
        if arm == 3 or arm < 0 or arm > 6:
            earth = earth_rgb8()
            eh, ew = earth.shape[:2]
        h = _P()
        d = (C.c_uint32 * 3)()
        _ck(_lib.rt1w_scene_build_reference(arm, C.c_uint64(build_seed), aspect_ratio,
                                            earth.ctypes.data_as(_P) if earth is not None else None,
                                            ew, eh, C.byref(h), C.byref(d)))
        return cls(_handle=h, _defaults=(d[0], d[1], d[2]))

    # draws from the build stream
    def rng_f64(self):
        x = C.c_double()
        _ck(_lib.rt1w_scene_rng_f64(self._h, C.byref(x)))
        return x.value

    def rng_range(self, lo, hi):
        x = C.c_double()
        _ck(_lib.rt1w_scene_rng_range(self._h, lo, hi, C.byref(x)))
        return x.value

    # textures
    def solid_color(self, rgb): return _ck(_lib.rt1w_texture_solid(self._h, _v3(rgb)))
    def checker_texture(self, odd, even): return _ck(_lib.rt1w_texture_checker(self._h, odd, even))
    def noise_texture(self, scale): return _ck(_lib.rt1w_texture_noise(self._h, scale))

    def noise_texture_tables(self, scale, ranvec, perm_x, perm_y, perm_z):
        rv = np.ascontiguousarray(ranvec, dtype=np.float64).reshape(768)
        ps = [np.ascontiguousarray(p, dtype=np.uint32).reshape(256) for p in (perm_x, perm_y, perm_z)]
        return _ck(_lib.rt1w_texture_noise_tables(self._h, scale, rv.ctypes.data_as(_P), *[p.ctypes.data_as(_P) for p in ps]))

    def image_texture(self, rgb8):
        a = np.ascontiguousarray(rgb8, dtype=np.uint8)
        h, w = a.shape[:2]
        return _ck(_lib.rt1w_texture_image(self._h, a.ctypes.data_as(_P), w, h))

    # materials
    def lambertian(self, tex): return _ck(_lib.rt1w_material_lambertian(self._h, tex))
    def metal(self, albedo, fuzz): return _ck(_lib.rt1w_material_metal(self._h, _v3(albedo), fuzz))
    def dielectric(self, ir): return _ck(_lib.rt1w_material_dielectric(self._h, ir))
    def diffuse_light(self, tex): return _ck(_lib.rt1w_material_diffuse_light(self._h, tex))
    def null_material(self): return _ck(_lib.rt1w_material_null(self._h))

    # hittables
    def sphere(self, center, radius, mat): return _ck(_lib.rt1w_hittable_sphere(self._h, _v3(center), radius, mat))

    def moving_sphere(self, c0, c1, t0, t1, radius, mat):
        return _ck(_lib.rt1w_hittable_moving_sphere(self._h, _v3(c0), _v3(c1), t0, t1, radius, mat))

    def xy_rect(self, x0, x1, y0, y1, k, mat): return _ck(_lib.rt1w_hittable_xy_rect(self._h, x0, x1, y0, y1, k, mat))
    def xz_rect(self, x0, x1, z0, z1, k, mat): return _ck(_lib.rt1w_hittable_xz_rect(self._h, x0, x1, z0, z1, k, mat))
    def yz_rect(self, y0, y1, z0, z1, k, mat): return _ck(_lib.rt1w_hittable_yz_rect(self._h, y0, y1, z0, z1, k, mat))
    def aabox(self, p0, p1, mat): return _ck(_lib.rt1w_hittable_aabox(self._h, _v3(p0), _v3(p1), mat))
    def translate(self, child, offset): return _ck(_lib.rt1w_hittable_translate(self._h, child, _v3(offset)))
    def rotate_y(self, child, angle_deg, time0=0.0, time1=1.0): return _ck(_lib.rt1w_hittable_rotate_y(self._h, child, time0, time1, angle_deg))
    def flip_face(self, child): return _ck(_lib.rt1w_hittable_flip_face(self._h, child))
    def constant_medium(self, boundary, density, tex): return _ck(_lib.rt1w_hittable_constant_medium(self._h, boundary, density, tex))

    def bvh_node(self, children, time0=0.0, time1=1.0):
        arr = (C.c_int * len(children))(*children)
        return _ck(_lib.rt1w_hittable_bvh(self._h, arr, len(children), time0, time1))

    # scene level
    def set_world(self, hid): _ck(_lib.rt1w_scene_set_world(self._h, hid))

    def set_lights(self, ids):
        arr = (C.c_int * max(1, len(ids)))(*ids)
        _ck(_lib.rt1w_scene_set_lights(self._h, arr, len(ids)))

    def set_background(self, rgb): _ck(_lib.rt1w_scene_set_background(self._h, _v3(rgb)))

    def set_camera(self, look_from, look_at, vup, vfov_deg, aspect_ratio, aperture, focus_dist, time0, time1):
        _ck(_lib.rt1w_scene_set_camera(self._h, _v3(look_from), _v3(look_at), _v3(vup), vfov_deg, aspect_ratio,
                                       aperture, focus_dist, time0, time1))

    def commit(self): _ck(_lib.rt1w_scene_commit(self._h))

    def set_bvh_build(self, mode):
        """Opt-in BVH build (rt1w_scene_set_bvh_build): False / 0 = BVHNode::new as written (random axis, median split; default),
        True / 1 / "sah" = the trees rebuilt by surface-area heuristic (statistically the same frames, not bit for bit),
        2 / "best_axis" = BVHNode::new as written with the axis of bvh.rs:84 chosen by the lowest cost of its median split instead of
        drawn (a tree the reference itself can build).  Returns self."""
        mode = {"reference": 0, "sah": 1, "best_axis": 2}.get(mode, mode)
        _ck(_lib.rt1w_scene_set_bvh_build(self._h, int(mode)))
        return self

    def set_walk_order(self, near_far):
        """Opt-in traversal order (rt1w_scene_set_walk_order): False = the reference's left-then-right (default),
        True = near child first in media-free subtrees.  On a committed scene, before creating contexts."""
        _ck(_lib.rt1w_scene_set_walk_order(self._h, int(near_far)))   # 0 reference, 1 near-far (frames identical on all tested scenes, not provably; segment counts may differ), 2 near-far everywhere
        return self

    def default_chunk(self, tile_w, tile_h, spp):
        """Samples per work item the renders of THIS scene use when `chunk` is 0 (rt1w_scene_default_chunk): 1 for scenes on the
        stack-walk kernels, the scene-independent rule (default_chunk) for the others."""
        return int(_lib.rt1w_scene_default_chunk(self._h, tile_w, tile_h, spp))

    def bvh_topology(self):
        """The trees of the opt-in SAH / best-axis builds as one int32 stream (rt1w_scene_get_bvh_topology); empty for the reference's build."""
        n = int(_lib.rt1w_scene_get_bvh_topology(self._h, None, 0))
        _ck(n)
        out = np.zeros(max(n, 1), dtype=np.int32)
        _ck(int(_lib.rt1w_scene_get_bvh_topology(self._h, out.ctypes.data_as(_P), n)))
        return out[:n]

    def info(self):
        i = SceneInfo()
        _ck(_lib.rt1w_scene_get_info(self._h, C.byref(i)))
        return {n: getattr(i, n) for n, _ in SceneInfo._fields_}

    def kernel_key(self, tiles=False):
        """Cache key of this scene's specialised kernel (sweep_<key>.hsaco); raises ERR_UNSUPPORTED for big scenes.
        tiles: the key of the kernel's tile-list form (rt1w_scene_kernel_key_tiles)."""
        buf = (C.c_char * 24)()
        _ck((_lib.rt1w_scene_kernel_key_tiles if tiles else _lib.rt1w_scene_kernel_key)(self._h, buf))
        return buf.value.decode()

    def kernel_source(self, f32=False, tiles=False):
        """The translation unit generated for this scene's specialised kernel (struct TopoJit: kind, skip, reuse), as text.
        tiles: the unit of the kernel's tile-list form (rt1w_scene_kernel_source_tiles; f64 only)."""
        if tiles and f32:
            raise ValueError("the tile-list form of the specialised kernel is f64 only")
        ask = (lambda buf, cap: _lib.rt1w_scene_kernel_source_tiles(self._h, buf, cap)) if tiles else \
              (lambda buf, cap: _lib.rt1w_scene_kernel_source(self._h, int(f32), buf, cap))
        n = ask(None, 0)
        _ck(int(n))
        buf = C.create_string_buffer(int(n) + 1)
        _ck(int(ask(buf, int(n))))
        return buf.raw[:int(n)].decode()

    def flat(self, what):
        """Bytes of one flat array (0 nodes,1 lights,2 materials,3 textures,4 perlin,5 images,6 camera+bg)."""
        n = _lib.rt1w_scene_copy_flat(self._h, what, None, 0)
        _ck(int(n))
        buf = np.zeros(max(int(n), 1), dtype=np.uint8)
        _ck(int(_lib.rt1w_scene_copy_flat(self._h, what, buf.ctypes.data_as(_P), int(n))))
        return buf[:int(n)]


class Context:
    """One GPU + one HIP stream with the scene uploaded (rt1w_context)."""

    def __init__(self, scene, device=0):
        h = _P()
        _ck(_lib.rt1w_context_create(device, scene._h, C.byref(h)))
        self._h = h
        self.scene = scene
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            _lib.rt1w_context_destroy(self._h)
            self._h = None

    __del__ = close

    @staticmethod
    def _params(width, height, spp, max_depth, tile, sample_offset, global_seed, chunk, out_sum, *, variant=None, strips=None, f32=False,
                partial_mib=0, flags=0, **switches):
        """rt1w_render_params.  switches: the keywords of _RENDER_FLAGS (out_sum is one of them); flags: raw RT1W_* bits on top."""
        if switches.keys() - _RENDER_FLAGS.keys():
            raise TypeError(f"_params() got an unexpected keyword argument {sorted(switches.keys() - _RENDER_FLAGS.keys())[0]!r}")
        if switches.get("wavefront"):
            load_lab()
        for name, on in dict(switches, out_sum=out_sum).items():
            flags |= _RENDER_FLAGS[name] if on else 0
        if variant is not None:
            flags |= (variant + 1) << 8
        x0, y0, tw, th = tile if tile is not None else (0, 0, width, height)
        sr, sp = strips if strips is not None else (0, 0)
        return RenderParams(width, height, x0, y0, tw, th, spp, sample_offset, max_depth, global_seed, chunk, flags, sr, sp, 1 if f32 else 0, int(partial_mib))

    def _composite(self, width, height, spp, max_depth, sample_offset, global_seed, chunk, flags, denoise, kw, filter=False, precision=None):
        """(p, d, out) of the entries that render and filter in one call.  kw: Context.render's keywords, `tile` among them; flags: raw
        RT1W_* render flags; denoise: dict of the filter's keywords -- without one d is None (the defaults), unless `filter` asks for
        the filter; precision: rt1w_render_params.precision, None = what kw's f32 says."""
        p = self._params(width, height, spp, max_depth, kw.pop("tile", None), sample_offset, global_seed, chunk, False, flags=flags, **kw)
        if precision is not None:
            p.precision = precision
        d = _denoise_params(0, 0, **(denoise or {})) if (filter or denoise is not None) else None
        return p, d, np.empty((p.tile_h, p.tile_w, 3), dtype=np.float64)

    def _entry(self, fn, prep, with_stats):
        """A feature entry on host arrays: `prep` = (arguments, results) of the entry's _*_prep.  Returns the results, with the stats
        dict after them if asked for."""
        args, out = prep
        return _ret(out, _call(fn, self._h, *args), with_stats)

    def specialise(self, cached_only=False, tiles=False):
        """Load (from the kernel cache) or compile (hiprtc, 3-5 s) the kernel specialised for this scene's topology
        (rt1w_context_specialise).  Returns the info dict; raises Rt1wError for scenes of more than 256 nodes
        (ERR_UNSUPPORTED) or, with cached_only, on a cache miss (ERR_STATE).  tiles: the kernel's tile-list form too
        (RT1W_SPECIALISE_TILES: what render_tiles(specialised=True) runs)."""
        info = SpecialiseInfo()
        _call(_lib.rt1w_context_specialise, self._h, (SPECIALISE_CACHED_ONLY if cached_only else 0) | (SPECIALISE_TILES if tiles else 0), info, stats=False)
        return {"key": info.key.decode(), "active": bool(info.active), "from_cache": bool(info.from_cache),
                "compile_ms": info.compile_ms, "grid": info.grid, "vgprs": info.vgprs}

    def specialised(self):
        """True if renders on this context use a scene-specialised kernel (cache hit at creation or specialise())."""
        info = SpecialiseInfo()
        rc = _lib.rt1w_context_specialise(self._h, SPECIALISE_CACHED_ONLY, C.byref(info))
        return rc == 0 and bool(info.active)

    def render(self, width, height, spp, max_depth=50, tile=None, sample_offset=0, global_seed=0, chunk=0, out_sum=False,
               variant=None, unsorted=False, lds_nodes=False, generic=False, wavefront=False, strips=None, out=None, frame=None,
               reference_stream=False, f32=False, classic_walk=False, probe_coherent=False, partial_mib=0, no_node_cache=False):
        """Returns (image[tile_h, tile_w, 3] float64 with row 0 = reference row j = y0, stats dict).
        probe_coherent: measurement mode RT1W_PROBE_COHERENT -- the returned array is NOT the image.
        strips=(strip_rows, strip_period): row-interleaved tile (tile row r = image row y0 + r//strip_rows*strip_period +
        r%strip_rows).  out: caller's array for the packed tile (e.g. pinned_empty).  frame: caller's WHOLE image
        [height, width, 3]; the tile's pixels are written at their image positions (RT1W_OUT_FRAME) and `frame` is returned."""
        p = self._params(width, height, spp, max_depth, tile, sample_offset, global_seed, chunk, out_sum, variant=variant, unsorted=unsorted,
                         lds_nodes=lds_nodes, generic=generic, wavefront=wavefront, strips=strips, out_frame=frame is not None,
                         reference_stream=reference_stream, f32=f32, classic_walk=classic_walk, probe_coherent=probe_coherent,
                         partial_mib=partial_mib, no_node_cache=no_node_cache)
        if frame is not None:
            assert frame.dtype == np.float64 and frame.shape == (height, width, 3) and frame.flags.c_contiguous
            out = frame
        elif out is None:
            out = np.empty((p.tile_h, p.tile_w, 3), dtype=np.float64)
        else:
            assert out.dtype == np.float64 and out.shape == (p.tile_h, p.tile_w, 3) and out.flags.c_contiguous
        return out, _call(_lib.rt1w_render, self._h, p, out)

    def render_u8(self, width, height, spp, max_depth=50, tile=None, sample_offset=0, global_seed=0, chunk=0, reference_stream=False,
                  partial_mib=0):
        """Quantised on the device, rows top-down as the reference prints them: uint8 [tile_h, tile_w, 3]."""
        p = self._params(width, height, spp, max_depth, tile, sample_offset, global_seed, chunk, False, reference_stream=reference_stream,
                         partial_mib=partial_mib)
        out = np.empty((p.tile_h, p.tile_w, 3), dtype=np.uint8)
        return out, _call(_lib.rt1w_render_u8, self._h, p, out)

    def render_rows(self, width, height, spp, strip_rows=0, u8=False, progress=None, max_depth=50, tile=None,
                    sample_offset=0, global_seed=0, chunk=0, out_sum=False, out=None, no_node_cache=False, partial_mib=0, f32=False, generic=False):
        """Strip-wise render from the top row down with D2H overlapped (rt1w_render_rows).  `progress(rows_done, rows_total)`
        is called as strips land; returning a true value cancels (raises Rt1wError with code ERR_CANCELLED).
        Returns the same arrays as render() (u8=False) or render_u8() (u8=True)."""
        p = self._params(width, height, spp, max_depth, tile, sample_offset, global_seed, chunk, out_sum, no_node_cache=no_node_cache,
                         partial_mib=partial_mib, f32=f32, generic=generic)
        if out is None:
            out = np.empty((p.tile_h, p.tile_w, 3), dtype=np.uint8 if u8 else np.float64)
        assert out.flags.c_contiguous and out.shape == (p.tile_h, p.tile_w, 3) and out.dtype == (np.uint8 if u8 else np.float64)
        cb = PROGRESS_FN((lambda user, done, total: 1 if progress(done, total) else 0) if progress else 0)
        return out, _call(_lib.rt1w_render_rows, self._h, p, strip_rows, ROWS_U8 if u8 else ROWS_F64, out, cb, None)

    def render_device(self, d_ptr, width, height, spp, max_depth=50, tile=None, sample_offset=0, global_seed=0, chunk=0,
                      out_sum=False, variant=None, unsorted=False, generic=False, strips=None, f32=False, partial_mib=0):
        """Same, into device memory `d_ptr` (int address, e.g. torch tensor .data_ptr()); packed tile rows."""
        p = self._params(width, height, spp, max_depth, tile, sample_offset, global_seed, chunk, out_sum, variant=variant, unsorted=unsorted,
                         generic=generic, strips=strips, f32=f32, partial_mib=partial_mib)
        return _call(_lib.rt1w_render_device, self._h, p, d_ptr)

    def render_tiles(self, width, height, spp, tile, tiles, max_depth=50, sample_offset=0, global_seed=0, chunk=0, out_sum=False, generic=False,
                     partial_mib=0, flags=0, strips=None, f32=False, specialised=False):
        """A list of square tiles of side `tile` in one launch (rt1w_render_tiles): `tiles` = Tile objects or (x0, y0, sample_offset)
        tuples.  Returns (float64 [n, tile, tile, 3], stats); tile k's row 0 = image row y0_k, pixels beyond the frame's edge are +0.0.
        specialised: RT1W_TILES_SPECIALISED -- the tile-list form of the scene-specialised kernel where a kernel cache has one."""
        p = self._params(width, height, spp, max_depth, None, sample_offset, global_seed, chunk, out_sum, generic=generic, partial_mib=partial_mib,
                         strips=strips, f32=f32, flags=flags | (TILES_SPECIALISED if specialised else 0))
        rec, n = _tile_list(tiles)
        out = np.empty((n, tile, tile, 3), dtype=np.float64)
        return out, _call(_lib.rt1w_render_tiles, self._h, p, tile, rec, n, out)

    def render_tiles_device(self, d_ptr, width, height, spp, tile, tiles, max_depth=50, sample_offset=0, global_seed=0, chunk=0, out_sum=False,
                            generic=False, partial_mib=0, flags=0, specialised=False):
        """Same, into device memory `d_ptr` (int address) of n * tile * tile * 3 doubles; the list itself is host memory.  Returns the stats."""
        p = self._params(width, height, spp, max_depth, None, sample_offset, global_seed, chunk, out_sum, generic=generic, partial_mib=partial_mib,
                         flags=flags | (TILES_SPECIALISED if specialised else 0))
        return _call(_lib.rt1w_render_tiles_device, self._h, p, tile, *_tile_list(tiles), d_ptr)

    def render_aov(self, width, height, spp, tile=None, sample_offset=0, global_seed=0, variant=None, strips=None, with_stats=False):
        """First-hit feature buffers of the tile (rt1w_render_aov): float64 [tile_h, tile_w, 8] = albedo rgb, normal xyz, depth,
        coverage, row 0 = reference row j = y0 (include/rt1w.h has the semantics).  with_stats: returns (array, stats dict)."""
        return self._entry(_lib.rt1w_render_aov, _aov_prep((), width, height, spp, tile, sample_offset, global_seed, variant, strips), with_stats)

    def render_aov_device(self, d_ptr, width, height, spp, tile=None, sample_offset=0, global_seed=0, variant=None, strips=None):
        """Same, into device memory `d_ptr` (int address of tile_h * tile_w * 8 float64, e.g. a torch tensor's .data_ptr());
        returns the stats dict."""
        p = self._params(width, height, spp, 0, tile, sample_offset, global_seed, 0, False, variant=variant, strips=strips)
        return _call(_lib.rt1w_render_aov_device, self._h, p, d_ptr)

    def render_aov_deep(self, width, height, spp, max_specular=8, max_fuzz=0.0, tile=None, sample_offset=0, global_seed=0, variant=None,
                        strips=None, with_stats=False):
        """Deep feature buffers of the tile (rt1w_render_aov_deep): the 8 channels of render_aov at the first vertex of each sample's
        path that is neither a Dielectric nor a Metal of fuzz <= max_fuzz, after at most max_specular bounces.  stats["segments"] is
        the number of rays traced."""
        return self._entry(_lib.rt1w_render_aov_deep,
                           _aov_prep((max_specular, max_fuzz), width, height, spp, tile, sample_offset, global_seed, variant, strips), with_stats)

    def render_aov_deep_device(self, d_ptr, width, height, spp, max_specular=8, max_fuzz=0.0, tile=None, sample_offset=0, global_seed=0,
                               variant=None, strips=None):
        """Same, into device memory `d_ptr` (int address of tile_h * tile_w * 8 float64); returns the stats dict."""
        p = self._params(width, height, spp, 0, tile, sample_offset, global_seed, 0, False, variant=variant, strips=strips)
        return _call(_lib.rt1w_render_aov_deep_device, self._h, p, max_specular, max_fuzz, d_ptr)

    def hit(self, rays, t_min=0.001, t_max=float("inf"), first_stream=0, sample=0, global_seed=0, variant=None, with_stats=False):
        """Ray queries (rt1w_hit): Hittable::hit of the scene's world for the caller's rays [n, 9] = origin, direction, time, t_min,
        t_max -- or [n, 7] with `t_min` and `t_max` filled in.  Returns (records float64 [n, 12] = hit, t, p xyz, normal xyz, u, v,
        front_face, material id; nodes uint32 [n] = the hit leaf's index in Scene.flat(0), HIT_NO_NODE on a miss).  A medium's draws of
        ray r come from the stream of pixel seed first_stream + r (include/rt1w.h has the semantics)."""
        return self._entry(_lib.rt1w_hit, _hit_prep(rays, t_min, t_max, first_stream, sample, global_seed, variant), with_stats)

    def ray_color(self, rays, start_word=None, with_stats=False, **kw):
        """Radiance queries (rt1w_ray_color): ray_color of the scene for the caller's rays [n, 7] = origin, direction, time (or wider
        records, e.g. [n, 9] as hit() takes them) through the render kernels' ray-list form.  Returns float64 [n, 3]: the mean of spp
        samples per ray, or with out_sum their raw sum.  kw: spp=1, sample_offset=0, max_depth=50, first_stream=0, global_seed=0, chunk=0,
        out_sum, generic, partial_mib; f32=True is refused with ERR_UNSUPPORTED (the ray-list kernels are f64 only; rt1w_ray_color_params
        has no precision member, so this refusal is the binding's).  Sample k of ray r draws from the stream of pixel seed first_stream + r, sample sample_offset + k,
        from word start_word[r] on (None: word 0; include/rt1w.h has the semantics)."""
        return self._entry(_lib.rt1w_ray_color, _ray_color_prep(rays, start_word, kw), with_stats)

    def ray_color_device(self, d_rays, d_out, n, d_start_word=None, stride=RAY_RECORD, **kw):
        """Same on device memory of the context's GPU (int addresses, e.g. torch tensors' .data_ptr()): d_rays n * stride float64, d_out
        n * 3 float64, d_start_word None or n uint32; no host copy.  kw as ray_color's (f32=True: ERR_UNSUPPORTED, the binding's own
        refusal).  Returns the stats dict."""
        return _call(_lib.rt1w_ray_color_device, self._h, _ray_color_params(n, stride=stride, **kw), d_rays, d_start_word, d_out)

    def path_begin(self, width, height, pixels, global_seed=0, max_depth=50, device=False, out=None, with_stats=False):
        """Fresh path states from the context's live camera (rt1w_path_begin): pixels [n, 3] = i, j, sample -> a PATH_STATE array [n]
        holding the camera ray of that sample of pixel (i, j) of a width x height frame, beta 1, radiance 0, the stream and its position
        behind Camera::get_ray, depth_left = max_depth, status PATH_ALIVE.  device=True: `pixels` is an int32 tensor [n, 3] on the
        context's GPU, the states come back as a float64 tensor [n, 16] (`out`, or a new one) without a host copy."""
        if not device:
            return self._entry(_lib.rt1w_path_begin, _path_begin_prep(width, height, pixels, global_seed, max_depth), with_stats)
        import torch
        if pixels.dim() != 2 or pixels.shape[1] != 3 or pixels.element_size() != 4 or not pixels.is_contiguous() or not pixels.is_cuda:
            raise ValueError("pixels must be a contiguous int32 tensor [n, 3] on the GPU")
        if out is None:
            out = torch.empty((pixels.shape[0], 16), dtype=torch.float64, device=pixels.device)
        d_out, n = _path_tensor(out, "out")
        if n != pixels.shape[0]:
            raise ValueError("out must hold one state per pixel")
        return _ret(out, self.path_begin_device(pixels.data_ptr(), d_out, n, width, height, global_seed, max_depth), with_stats)

    def path_begin_device(self, d_pixels, d_out, n, width, height, global_seed=0, max_depth=50):
        """rt1w_path_begin_device on raw device addresses: d_pixels n * 3 uint32, d_out n states (16-byte aligned).  Returns the stats."""
        return _call(_lib.rt1w_path_begin_device, self._h, width, height, global_seed, max_depth, d_pixels, n, d_out)

    def path_step(self, states, steps=1, global_seed=0, variant=None, device=False, nodes=None, with_stats=False):
        """Path states advanced by up to `steps` levels of ray_color each (rt1w_path_step): states = a PATH_STATE array [n] (or float64
        [n, 16]).  Returns (the advanced states, uint32 [n] = the hit leaf of each state's last level, PATH_NO_NODE for none); the input
        is left as it was.  A dead state comes back unchanged.  device=True: `states` is a float64 tensor [n, 16] on the context's GPU
        and is advanced IN PLACE, taken by pointer (`nodes`: an optional int32 tensor [n] for the leaves); returns the stats."""
        if not device:
            return self._entry(_lib.rt1w_path_step, _path_step_prep(states, steps, global_seed, variant), with_stats)
        d_states, n = _path_tensor(states, "states")
        if nodes is not None and (nodes.dim() != 1 or nodes.shape[0] != n or nodes.element_size() != 4 or not nodes.is_contiguous() or not nodes.is_cuda):
            raise ValueError("nodes must be a contiguous int32 tensor [n] on the GPU")
        return self.path_step_device(d_states, d_states, None if nodes is None else nodes.data_ptr(), n, steps, global_seed, variant)

    def path_step_device(self, d_in, d_out, d_node, n, steps=1, global_seed=0, variant=None):
        """rt1w_path_step_device on raw device addresses: d_in, d_out n states (16-byte aligned; the same address or apart), d_node None
        or n uint32.  Returns the stats."""
        return _call(_lib.rt1w_path_step_device, self._h, _path_params(n, steps, global_seed, variant), d_in, d_out, d_node)

    def hit_device(self, d_rays, d_out, d_node, n, first_stream=0, sample=0, global_seed=0, variant=None):
        """Same on device memory (int addresses, e.g. torch tensors' .data_ptr()): d_rays n * 9 float64 with the bounds in, d_out n * 12
        float64, d_node n uint32 or None; returns the stats dict."""
        return _call(_lib.rt1w_hit_device, self._h, _hit_params(n, first_stream, sample, global_seed, variant), d_rays, d_out, d_node)

    def denoise(self, frame, aov, with_stats=False, **kw):
        """Feature-guided filter (rt1w_denoise) of a float64 frame [h, w, 3] with its feature buffers [h, w, 8] (render_aov): the
        denoised [h, w, 3].  kw: iterations, keep_albedo, sigma_colour, sigma_normal, sigma_depth (0 = default)."""
        return self._entry(_lib.rt1w_denoise, _denoise_prep(frame, aov, kw), with_stats)

    def denoise_device(self, d_frame, d_aov, d_out, width, height, **kw):
        """Same on device memory (int addresses of height * width * 3 / 8 / 3 float64, e.g. torch tensors' .data_ptr()); d_out may
        equal d_frame.  Returns the stats dict."""
        return _call(_lib.rt1w_denoise_device, self._h, _denoise_params(width, height, **kw), d_frame, d_aov, d_out)

    def set_camera(self, look_from, look_at, vup, vfov_deg, aspect_ratio, aperture, focus_dist, time0, time1):
        """Replace this context's camera (rt1w_context_set_camera): Scene.set_camera's arguments and arithmetic, host work only.
        The scene and its other contexts keep theirs."""
        _call(_lib.rt1w_context_set_camera, self._h, _v3(look_from), _v3(look_at), _v3(vup), vfov_deg, aspect_ratio, aperture, focus_dist,
              time0, time1, stats=False)

    def get_camera(self):
        """The Camera the kernels of this context are handed now (rt1w_context_get_camera)."""
        cam = Camera()
        _call(_lib.rt1w_context_get_camera, self._h, cam, stats=False)
        return cam

    def temporal_accumulate(self, cur_frame, cur_aov, cur_cam, prev_hist, prev_len, prev_aov, prev_cam, with_stats=False, **kw):
        """Temporal accumulation (rt1w_temporal_accumulate) of a float64 frame [h, w, 3] with its feature buffers [h, w, 8] against the
        previous frame's (hist [h, w, 3], len [h, w], feature buffers); the cameras are Camera or 24 doubles.  Returns
        (hist, len, frame_out).  kw: keep_albedo, max_history, depth_tol, normal_min (0 = default)."""
        return self._entry(_lib.rt1w_temporal_accumulate, _temporal_prep(cur_frame, cur_aov, cur_cam, prev_hist, None, prev_len, prev_aov, prev_cam, kw),
                           with_stats)

    def temporal_accumulate_device(self, d_cur_frame, d_cur_aov, cur_cam, d_prev_hist, d_prev_len, d_prev_aov, prev_cam, d_hist, d_len,
                                   d_frame_out, width, height, **kw):
        """Same on device memory (int addresses, e.g. torch tensors' .data_ptr()).  Returns the stats dict."""
        return _call(_lib.rt1w_temporal_accumulate_device, self._h, _temporal_params(width, height, **kw), d_cur_frame, d_cur_aov, Camera.of(cur_cam),
                     d_prev_hist, d_prev_len, d_prev_aov, Camera.of(prev_cam), d_hist, d_len, d_frame_out)

    def render_temporal(self, width, height, spp, max_depth=50, sample_offset=0, global_seed=0, temporal=None, denoise=None, filter=False,
                        flags=0, with_stats=False, **kw):
        """One frame of an animation (rt1w_render_temporal): render, feature buffers, accumulation against the state this context keeps
        from the previous call, optionally the filter (filter=True, or `denoise`: dict of Context.denoise's keywords): float64
        [height, width, 3].  `temporal`: dict of temporal_accumulate's keywords; other kw as Context.render's."""
        p, d, out = self._composite(width, height, spp, max_depth, sample_offset, global_seed, 0, flags, denoise, kw, filter=filter)
        t = _temporal_params(0, 0, **temporal) if temporal is not None else None
        return _ret(out, _call(_lib.rt1w_render_temporal, self._h, p, t, d, out), with_stats)

    def temporal_moments(self, cur_frame, cur_aov, cur_cam, prev_hist, prev_m2, prev_len, prev_aov, prev_cam, with_stats=False, **kw):
        """temporal_accumulate with the second-moment channel (rt1w_temporal_moments): prev_m2 [h, w] goes in after prev_hist, and
        (hist, m2, len, frame_out) come back; hist, len and frame_out are temporal_accumulate's bits.  kw as temporal_accumulate's."""
        return self._entry(_lib.rt1w_temporal_moments, _temporal_prep(cur_frame, cur_aov, cur_cam, prev_hist, prev_m2, prev_len, prev_aov, prev_cam, kw),
                           with_stats)

    def temporal_moments_device(self, d_cur_frame, d_cur_aov, cur_cam, d_prev_hist, d_prev_m2, d_prev_len, d_prev_aov, prev_cam, d_hist, d_m2,
                                d_len, d_frame_out, width, height, **kw):
        """Same on device memory (int addresses, e.g. torch tensors' .data_ptr()).  Returns the stats dict."""
        return _call(_lib.rt1w_temporal_moments_device, self._h, _temporal_params(width, height, **kw), d_cur_frame, d_cur_aov, Camera.of(cur_cam),
                     d_prev_hist, d_prev_m2, d_prev_len, d_prev_aov, Camera.of(prev_cam), d_hist, d_m2, d_len, d_frame_out)

    def temporal_variance(self, hist, m2, length, aov, with_stats=False):
        """The variance buffer of denoise_var from a history (rt1w_temporal_variance): hist [h, w, 3], m2 and len [h, w] as
        temporal_moments returned them, aov the CURRENT frame's feature buffers: var [h, w]."""
        return self._entry(_lib.rt1w_temporal_variance, _temporal_variance_prep(hist, m2, length, aov), with_stats)

    def temporal_variance_device(self, d_hist, d_m2, d_len, d_aov, d_var, width, height):
        """Same on device memory (int addresses).  Returns the stats dict."""
        return _call(_lib.rt1w_temporal_variance_device, self._h, width, height, d_hist, d_m2, d_len, d_aov, d_var)

    def render_temporal_var(self, width, height, spp, max_depth=50, sample_offset=0, global_seed=0, temporal=None, denoise=None,
                            sigma_variance=0.0, flags=0, with_stats=False, **kw):
        """One frame of an animation filtered with the history's own variance (rt1w_render_temporal_var): render, feature buffers,
        temporal_moments against a state of this entry's own, temporal_variance, denoise_var: float64 [height, width, 3].  `temporal`:
        dict of temporal_accumulate's keywords, `denoise`: dict of Context.denoise's; other kw as Context.render's."""
        p, d, out = self._composite(width, height, spp, max_depth, sample_offset, global_seed, 0, flags, denoise, kw)
        t = _temporal_params(0, 0, **temporal) if temporal is not None else None
        return _ret(out, _call(_lib.rt1w_render_temporal_var, self._h, p, t, d, sigma_variance, out), with_stats)

    def temporal_reset(self):
        """Forget the history of render_temporal and of render_temporal_var (rt1w_temporal_reset): the next call is a first frame."""
        _ck(_lib.rt1w_temporal_reset(self._h))

    def render_denoised(self, width, height, spp, max_depth=50, tile=None, sample_offset=0, global_seed=0, denoise=None, flags=0,
                        strips=None, precision=0, with_stats=False, **kw):
        """Render, feature buffers and filter in one call (rt1w_render_denoised): float64 [tile_h, tile_w, 3].  `denoise`: dict of
        the keywords of Context.denoise, None = defaults; `flags`: raw RT1W_* render flags; other kw as Context.render's."""
        p, d, out = self._composite(width, height, spp, max_depth, sample_offset, global_seed, 0, flags, denoise, dict(kw, tile=tile, strips=strips),
                                    precision=precision)
        return _ret(out, _call(_lib.rt1w_render_denoised, self._h, p, d, out), with_stats)

    def render_denoised_deep(self, width, height, spp, max_specular=8, max_fuzz=0.0, max_depth=50, tile=None, sample_offset=0, global_seed=0,
                             denoise=None, flags=0, strips=None, precision=0, with_stats=False, **kw):
        """render_denoised with the deep feature buffers (rt1w_render_denoised_deep) in place of the first-hit ones."""
        p, d, out = self._composite(width, height, spp, max_depth, sample_offset, global_seed, 0, flags, denoise, dict(kw, tile=tile, strips=strips),
                                    precision=precision)
        return _ret(out, _call(_lib.rt1w_render_denoised_deep, self._h, p, d, max_specular, max_fuzz, out), with_stats)

    def batch_variance(self, sums, aov, batch_spp, keep_albedo=False, with_stats=False):
        """Frame and variance from K sample batches (rt1w_batch_variance): `sums` float64 [K, h, w, 3], the raw sums of K renders with
        out_sum=True, spp=batch_spp and sample_offset = k * batch_spp; `aov` [h, w, 8].  Returns (frame [h, w, 3], var [h, w]): the mean
        over all K * batch_spp samples and the variance of the mean demodulated luminance."""
        return self._entry(_lib.rt1w_batch_variance, _batch_variance_prep(sums, aov, batch_spp, keep_albedo), with_stats)

    def batch_variance_device(self, d_sums, d_aov, d_frame, d_var, width, height, batches, batch_spp, keep_albedo=False):
        """Same on device memory (int addresses of batches * height * width * 3, height * width * 8 / 3 / 1 float64).  Returns the stats dict."""
        return _call(_lib.rt1w_batch_variance_device, self._h, width, height, batches, batch_spp, _keep(keep_albedo), d_sums, d_aov, d_frame, d_var)

    def denoise_var(self, frame, aov, var, sigma_variance=0.0, with_stats=False, **kw):
        """Variance-guided filter (rt1w_denoise_var) of a float64 frame [h, w, 3] with its feature buffers [h, w, 8] and the variance
        [h, w] of batch_variance: the denoised [h, w, 3].  kw: iterations, keep_albedo, sigma_normal, sigma_depth (0 = default)."""
        return self._entry(_lib.rt1w_denoise_var, _denoise_var_prep(frame, aov, var, sigma_variance, kw), with_stats)

    def denoise_var_device(self, d_frame, d_aov, d_var, d_out, width, height, sigma_variance=0.0, **kw):
        """Same on device memory (int addresses of height * width * 3 / 8 / 1 / 3 float64); d_out may equal d_frame.  Returns the stats dict."""
        return _call(_lib.rt1w_denoise_var_device, self._h, _denoise_params(width, height, **kw), d_frame, d_aov, d_var, sigma_variance, d_out)

    def render_denoised_var(self, width, height, spp, batches=0, sigma_variance=0.0, max_specular=0, max_fuzz=0.0, max_depth=50, tile=None,
                            sample_offset=0, global_seed=0, chunk=0, denoise=None, flags=0, strips=None, precision=0, with_stats=False, **kw):
        """Batches, feature buffers, batch variance and the variance-guided filter in one call (rt1w_render_denoised_var): float64
        [tile_h, tile_w, 3].  `spp` must be a multiple of `batches` (0 = 4); max_specular > 0 takes the deep feature buffers; other
        arguments as render_denoised."""
        p, d, out = self._composite(width, height, spp, max_depth, sample_offset, global_seed, chunk, flags, denoise, dict(kw, tile=tile, strips=strips),
                                    precision=precision)
        return _ret(out, _call(_lib.rt1w_render_denoised_var, self._h, p, d, batches, sigma_variance, max_specular, max_fuzz, out), with_stats)

    def accum_merge(self, acc, tile_sums, aov, batch_spp, x0=0, y0=0, keep_albedo=False, with_stats=False):
        """One rendered batch of a rectangle into an accumulator (rt1w_accum_merge): `acc` float64 [h, w, 8] (zeros = empty), `tile_sums`
        [tile_h, tile_w, 3] the raw sums of a render with out_sum=True, spp=batch_spp of the rectangle at (x0, y0), `aov` [h, w, 8] of the
        whole frame.  Returns the merged accumulator (a new array)."""
        return self._entry(_lib.rt1w_accum_merge, _merge_prep(acc, tile_sums, aov, batch_spp, x0, y0, keep_albedo), with_stats)

    def accum_merge_device(self, d_acc, d_tile_sums, d_aov, width, height, rect, batch_spp, keep_albedo=False):
        """Same on device memory (int addresses); rect = (x0, y0, tile_w, tile_h).  Returns the stats dict."""
        return _call(_lib.rt1w_accum_merge_device, self._h, width, height, *rect, batch_spp, _keep(keep_albedo), d_tile_sums, d_aov, d_acc)

    def accum_merge_tiles(self, acc, tile_sums, aov, batch_spp, tile, tiles, keep_albedo=False, with_stats=False):
        """One rendered batch of a LIST of square tiles into an accumulator in one launch (rt1w_accum_merge_tiles): `tile_sums`
        [n, tile, tile, 3] as render_tiles(out_sum=True) returns them, `tiles` its list.  Returns the merged accumulator (a new array)."""
        return self._entry(_lib.rt1w_accum_merge_tiles, _merge_tiles_prep(acc, tile_sums, aov, batch_spp, tile, tiles, keep_albedo), with_stats)

    def accum_merge_tiles_device(self, d_acc, d_tile_sums, d_aov, width, height, tile, tiles, batch_spp, keep_albedo=False):
        """Same on device memory (int addresses); the list itself is host memory.  Returns the stats dict."""
        return _call(_lib.rt1w_accum_merge_tiles_device, self._h, width, height, tile, *_tile_list(tiles), batch_spp, _keep(keep_albedo), d_tile_sums,
                     d_aov, d_acc)

    def accum_resolve(self, acc, batch_spp, with_stats=False):
        """(frame [h, w, 3], var [h, w], spp [h, w]) of an accumulator (rt1w_accum_resolve)."""
        return self._entry(_lib.rt1w_accum_resolve, _accum_resolve_prep(acc, batch_spp), with_stats)

    def accum_resolve_device(self, d_acc, d_frame, d_var, d_spp, width, height, batch_spp):
        return _call(_lib.rt1w_accum_resolve_device, self._h, width, height, batch_spp, d_acc, d_frame, d_var, d_spp)

    def accum_tile_error(self, acc, tile, with_stats=False):
        """The error of every tile of an accumulator (rt1w_accum_tile_error): float64 [ceil(h / tile), ceil(w / tile)]."""
        return self._entry(_lib.rt1w_accum_tile_error, _tile_error_prep(_accum_of(acc), tile), with_stats)

    def accum_tile_error_device(self, d_acc, d_err, width, height, tile):
        return _call(_lib.rt1w_accum_tile_error_device, self._h, width, height, tile, d_acc, d_err)

    def render_adaptive(self, width, height, adaptive=None, denoise=None, filter=False, sigma_variance=0.0, max_depth=50, sample_offset=0,
                        global_seed=0, chunk=0, tile=None, flags=0, strips=None, precision=0, with_stats=False, **kw):
        """Adaptive sampling in one call (rt1w_render_adaptive): (frame [h, w, 3], spp [h, w]).  `adaptive`: dict of the keywords of
        adaptive_params, None = defaults; `filter` or a `denoise` dict (keywords of Context.denoise_var) adds the variance-guided filter."""
        p, d, out = self._composite(width, height, 0, max_depth, sample_offset, global_seed, chunk, flags, denoise, dict(kw, tile=tile, strips=strips),
                                    filter=filter, precision=precision)
        spp = np.empty(out.shape[:2], dtype=np.float64)
        return _ret((out, spp), _call(_lib.rt1w_render_adaptive, self._h, p, adaptive_params(**(adaptive or {})), d, sigma_variance, out, spp), with_stats)

    def halves_resolve(self, acc_a, acc_b, batch_spp, with_stats=False):
        """(frame [h, w, 3], var [h, w], half_a [h, w, 3], half_b [h, w, 3], spp [h, w]) of two accumulators taken as the halves of one
        frame (rt1w_halves_resolve)."""
        return self._entry(_lib.rt1w_halves_resolve, _halves_resolve_prep(acc_a, acc_b, batch_spp), with_stats)

    def halves_resolve_device(self, d_acc_a, d_acc_b, d_frame, d_var, d_half_a, d_half_b, d_spp, width, height, batch_spp):
        """Same on device memory (int addresses).  Returns the stats dict."""
        return _call(_lib.rt1w_halves_resolve_device, self._h, width, height, batch_spp, d_acc_a, d_acc_b, d_frame, d_var, d_half_a, d_half_b, d_spp)

    def denoise_var_halves(self, frame, aov, var, half_a, half_b, sigma_variance=0.0, with_stats=False, **kw):
        """The variance-guided filter carrying the frame's two halves (rt1w_denoise_var_halves): (out [h, w, 3] -- the bits of denoise_var --
        and err_px [h, w], the half-buffer error of the filtered frame).  kw as denoise_var."""
        return self._entry(_lib.rt1w_denoise_var_halves, _halves_filter_prep(frame, aov, var, half_a, half_b, sigma_variance, kw), with_stats)

    def denoise_cross(self, frame, aov, var, half_a, half_b, sigma_variance=0.0, with_stats=False, **kw):
        """The two halves, each filtered with the other's colour term (rt1w_denoise_cross): (out [h, w, 3], the mean of the two filtered
        halves -- NOT the bits of denoise_var -- and err_px [h, w], their squared difference as the error of that frame).  kw as denoise_var."""
        return self._entry(_lib.rt1w_denoise_cross, _halves_filter_prep(frame, aov, var, half_a, half_b, sigma_variance, kw), with_stats)

    def denoise_var_halves_device(self, d_frame, d_aov, d_var, d_half_a, d_half_b, d_out, d_err_px, width, height, sigma_variance=0.0, **kw):
        """Same on device memory (int addresses); d_out may equal d_frame.  Returns the stats dict."""
        return _call(_lib.rt1w_denoise_var_halves_device, self._h, _denoise_params(width, height, **kw), d_frame, d_aov, d_var, d_half_a, d_half_b,
                     sigma_variance, d_out, d_err_px)

    def denoise_cross_device(self, d_frame, d_aov, d_var, d_half_a, d_half_b, d_out, d_err_px, width, height, sigma_variance=0.0, **kw):
        """Context.denoise_cross on device memory (int addresses); d_out may equal d_frame.  Returns the stats dict."""
        return _call(_lib.rt1w_denoise_cross_device, self._h, _denoise_params(width, height, **kw), d_frame, d_aov, d_var, d_half_a, d_half_b,
                     sigma_variance, d_out, d_err_px)

    def tile_error_map(self, err_px, tile, with_stats=False):
        """The tile means of a per-pixel error map (rt1w_tile_error_map): float64 [ceil(h / tile), ceil(w / tile)]."""
        return self._entry(_lib.rt1w_tile_error_map, _tile_error_prep(_error_map_of(err_px), tile), with_stats)

    def tile_error_map_device(self, d_err_px, d_err, width, height, tile):
        return _call(_lib.rt1w_tile_error_map_device, self._h, width, height, tile, d_err_px, d_err)

    def render_adaptive_filtered(self, width, height, adaptive=None, denoise=None, sigma_variance=0.0, max_depth=50, sample_offset=0, global_seed=0,
                                 chunk=0, tile=None, flags=0, strips=None, precision=0, with_stats=False, **kw):
        """Adaptive sampling steered by the filtered frame's half-buffer error, in one call (rt1w_render_adaptive_filtered): (filtered frame
        [h, w, 3], spp [h, w], err_px [h, w]).  `adaptive`: dict of the keywords of adaptive_params (pilot_batches even), None = defaults;
        `denoise`: dict of the keywords of Context.denoise_var, None = defaults."""
        return self._render_adaptive_halves(_lib.rt1w_render_adaptive_filtered, width, height, adaptive, denoise, sigma_variance, max_depth, sample_offset,
                                            global_seed, chunk, tile, flags, strips, precision, with_stats, kw)

    def render_adaptive_cross(self, width, height, adaptive=None, denoise=None, sigma_variance=0.0, max_depth=50, sample_offset=0, global_seed=0,
                              chunk=0, tile=None, flags=0, strips=None, precision=0, with_stats=False, **kw):
        """render_adaptive_filtered with the cross filter (rt1w_render_adaptive_cross): every round's estimate is Context.denoise_cross, so the
        frame is the mean of the two cross-filtered halves and err_px their squared difference.  Same arguments and results."""
        return self._render_adaptive_halves(_lib.rt1w_render_adaptive_cross, width, height, adaptive, denoise, sigma_variance, max_depth, sample_offset,
                                            global_seed, chunk, tile, flags, strips, precision, with_stats, kw)

    def _render_adaptive_halves(self, fn, width, height, adaptive, denoise, sigma_variance, max_depth, sample_offset, global_seed, chunk, tile, flags,
                                strips, precision, with_stats, kw):
        p, d, out = self._composite(width, height, 0, max_depth, sample_offset, global_seed, chunk, flags, denoise, dict(kw, tile=tile, strips=strips),
                                    precision=precision)
        spp, err = np.empty(out.shape[:2], dtype=np.float64), np.empty(out.shape[:2], dtype=np.float64)
        return _ret((out, spp, err), _call(fn, self._h, p, adaptive_params(**(adaptive or {})), d, sigma_variance, out, spp, err), with_stats)

    def render_aov_tiles(self, width, height, spp, tile, tiles, sample_offset=0, global_seed=0, variant=None, flags=0, strips=None, f32=False,
                         with_stats=False):
        """First-hit feature SUMS of a list of square tiles in one launch (rt1w_render_aov_tiles): `tiles` = Tile objects or (x0, y0,
        sample_offset) tuples.  Returns float64 [n, tile, tile, 8]: the sums of albedo rgb, normal xyz, t |d| over the hits and the hit count;
        tile k's row 0 = image row y0_k, pixels beyond the frame's edge are +0.0.  with_stats: returns (array, stats dict)."""
        return self._entry(_lib.rt1w_render_aov_tiles,
                           _aov_tiles_prep(width, height, spp, tile, tiles, sample_offset, global_seed, variant, flags, strips, f32), with_stats)

    def render_aov_tiles_device(self, d_ptr, width, height, spp, tile, tiles, sample_offset=0, global_seed=0, variant=None):
        """Same, into device memory `d_ptr` (int address) of n * tile * tile * 8 doubles; the list itself is host memory.  Returns the stats."""
        p = self._params(width, height, spp, 0, None, sample_offset, global_seed, 0, False, variant=variant)
        return _call(_lib.rt1w_render_aov_tiles_device, self._h, p, tile, *_tile_list(tiles), d_ptr)

    def guides_merge_tiles(self, gacc, tile_sums, spp, tile, tiles, with_stats=False):
        """The feature sums of a list of disjoint tiles into a guide accumulator (rt1w_guides_merge_tiles): `gacc` float64 [h, w, 9] (zeros =
        empty), `tile_sums` [n, tile, tile, 8] as render_aov_tiles returns them for `spp` samples.  Returns the merged accumulator (a new array)."""
        return self._entry(_lib.rt1w_guides_merge_tiles, _guides_merge_prep(gacc, tile_sums, spp, tile, tiles), with_stats)

    def guides_merge_tiles_device(self, d_gacc, d_tile_sums, width, height, tile, tiles, spp):
        """Same on device memory (int addresses); the list itself is host memory.  Returns the stats dict."""
        return _call(_lib.rt1w_guides_merge_tiles_device, self._h, width, height, tile, *_tile_list(tiles), spp, d_tile_sums, d_gacc)

    def guides_resolve(self, gacc, with_stats=False):
        """The feature buffers [h, w, 8] of a guide accumulator, in render_aov's layout (rt1w_guides_resolve)."""
        return self._entry(_lib.rt1w_guides_resolve, _guides_resolve_prep(gacc), with_stats)

    def guides_resolve_device(self, d_gacc, d_aov, width, height):
        return _call(_lib.rt1w_guides_resolve_device, self._h, width, height, d_gacc, d_aov)

    def render_adaptive_guided(self, width, height, adaptive=None, denoise=None, sigma_variance=0.0, max_depth=50, sample_offset=0, global_seed=0,
                               chunk=0, tile=None, flags=0, strips=None, precision=0, with_stats=False, **kw):
        """render_adaptive_filtered with full-count guides (rt1w_render_adaptive_guided): every round tops up the first-hit feature sums of
        the tiles it takes, and the filter is guided by all the samples a pixel holds.  Same arguments and results."""
        return self._render_adaptive_halves(_lib.rt1w_render_adaptive_guided, width, height, adaptive, denoise, sigma_variance, max_depth, sample_offset,
                                            global_seed, chunk, tile, flags, strips, precision, with_stats, kw)

    def debug_aabb(self, cases):
        """cases[n, 14] = min3, max3, origin3, direction3, t_min, t_max -> (literal[n], fast[n]) from the device."""
        a = np.ascontiguousarray(cases, dtype=np.float64).reshape(-1, 14)
        lit = np.empty(a.shape[0], dtype=np.int32)
        fast = np.empty(a.shape[0], dtype=np.int32)
        _ck(_lib.rt1w_debug_aabb(self._h, a.ctypes.data_as(_P), lit.ctypes.data_as(_P), fast.ctypes.data_as(_P), a.shape[0]))
        return lit, fast

    def debug_texture(self, mode, tex, uvp):
        """uvp[n, 5] = u, v, p.xyz -> out[n, 3] from the device: mode 0 Texture::value of texture `tex`, 1 Perlin noise / turb of
        table `tex`, 2 sphere_uv(p) (rt1w_debug_texture)."""
        a = np.ascontiguousarray(uvp, dtype=np.float64).reshape(-1, 5)
        out = np.empty((a.shape[0], 3), dtype=np.float64)
        _ck(_lib.rt1w_debug_texture(self._h, mode, tex, a.ctypes.data_as(_P), out.ctypes.data_as(_P), a.shape[0]))
        return out

    def debug_stamps(self, reset=True):
        out = (C.c_uint64 * 16)()
        rc = _ck(_lib.rt1w_debug_stamps(self._h, C.byref(out), 1 if reset else 0))
        return rc, [int(v) for v in out]

    def debug_eval(self, fn, a, b):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        out = np.empty_like(a)
        _ck(_lib.rt1w_debug_eval(self._h, fn, a.ctypes.data_as(_P), b.ctypes.data_as(_P), out.ctypes.data_as(_P), a.size))
        return out


class _Pinned:
    def __init__(self, ptr): self.ptr = ptr
    def __del__(self):
        if self.ptr: _lib.rt1w_host_free(self.ptr); self.ptr = None


def pinned_empty(shape, dtype=np.float64):
    """numpy array over page-locked host memory (rt1w_host_alloc): device->host copies into it run at full PCIe rate."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = _P()
    _ck(_lib.rt1w_host_alloc(n, C.byref(p)))
    keep = _Pinned(p)
    buf = (C.c_uint8 * n).from_address(p.value)
    a = np.frombuffer(buf, dtype=dtype).reshape(shape)
    _PINNED_KEEP[id(buf)] = keep
    import weakref
    weakref.finalize(buf, _PINNED_KEEP.pop, id(buf), None)
    return a


_PINNED_KEEP = {}


def host_register(array):
    """Pin memory the caller owns (e.g. a shared-memory mapping several single-GPU processes fill)."""
    _ck(_lib.rt1w_host_register(C.c_void_p(array.ctypes.data), array.nbytes))


def host_unregister(array):
    _ck(_lib.rt1w_host_unregister(C.c_void_p(array.ctypes.data)))


def aov_host(scene, width, height, spp, tile=None, sample_offset=0, global_seed=0, variant=None, strips=None, max_specular=None,
             max_fuzz=0.0, with_stats=False):
    """CPU twin of Context.render_aov (librt1w_lab.so: rt1w_lab_aov_host, the same rt_aov.h built for the host): the array the GPU
    must equal bit for bit.  No GPU needed.  max_specular not None: the twin of Context.render_aov_deep (rt1w_lab_aov_deep_host,
    rt_aov_deep.h); with_stats then returns (array, {"segments": rays traced, "lengths": uint8 [tile_h, tile_w, spp] rays per sample})."""
    args, out = _aov_prep(() if max_specular is None else (max_specular, max_fuzz), width, height, spp, tile, sample_offset, global_seed, variant, strips)
    if max_specular is None:
        _call_lab("rt1w_lab_aov_host", scene._h, *args)
        return (out, {"segments": out.shape[0] * out.shape[1] * spp}) if with_stats else out
    seg = C.c_uint64()
    lengths = np.zeros(out.shape[:2] + (spp,), dtype=np.uint8) if with_stats else None
    _call_lab("rt1w_lab_aov_deep_host", scene._h, *args, C.byref(seg), lengths)
    return (out, {"segments": seg.value, "lengths": lengths}) if with_stats else out


def aov_tiles_host(scene, width, height, spp, tile, tiles, sample_offset=0, global_seed=0, variant=None, flags=0, strips=None, f32=False):
    """CPU twin of Context.render_aov_tiles (librt1w_lab.so: rt1w_lab_aov_tiles_host, rt_aov_tiles.h built for the host): the sums
    [n, tile, tile, 8] the GPU must equal bit for bit.  No GPU needed."""
    args, out = _aov_tiles_prep(width, height, spp, tile, tiles, sample_offset, global_seed, variant, flags, strips, f32)
    _call_lab("rt1w_lab_aov_tiles_host", scene._h, *args)
    return out


def hit_host(scene, rays, t_min=0.001, t_max=float("inf"), first_stream=0, sample=0, global_seed=0, variant=None):
    """CPU twin of Context.hit (librt1w_lab.so: rt1w_lab_hit_host, the same rt_hit.h built for the host): the (records, nodes) the GPU
    must equal bit for bit.  No GPU needed."""
    args, out = _hit_prep(rays, t_min, t_max, first_stream, sample, global_seed, variant)
    return _twin("rt1w_lab_hit_host", ((scene._h, *args), out))


def texture_host(scene, mode, tex, uvp):
    """CPU twin of Context.debug_texture (librt1w_lab.so: rt1w_lab_texture_host, the same rt_core.h functions built for the host) over a
    committed scene: uvp[n, 5] = u, v, p.xyz -> out[n, 3], the array the GPU must equal bit for bit.  No GPU needed."""
    a = np.ascontiguousarray(uvp, dtype=np.float64).reshape(-1, 5)
    out = np.empty((a.shape[0], 3), dtype=np.float64)
    return _twin("rt1w_lab_texture_host", ((scene._h, mode, tex, a, out, a.shape[0]), out), says_why=True)


def camera_rays_host(scene, width, height, spp, tile=None, sample_offset=0, global_seed=0, strips=None):
    """The camera rays of a tile (librt1w_lab.so: rt1w_lab_camera_rays_host): float64 [tile_h, tile_w, spp, 8] = origin, direction, time,
    1 of the ray every sample's path and feature buffers begin with.  No GPU needed."""
    p = Context._params(width, height, spp, 0, tile, sample_offset, global_seed, 0, False, strips=strips)
    out = np.empty((p.tile_h, p.tile_w, spp, 8), dtype=np.float64)
    return _twin("rt1w_lab_camera_rays_host", ((scene._h, p, out), out))


def camera_rays_pos_host(scene, width, height, spp, tile=None, sample_offset=0, global_seed=0, strips=None):
    """camera_rays_host's rays and, per ray, uint32 [tile_h, tile_w, spp]: the word its sample's stream stands at behind the camera's
    draws (librt1w_lab.so: rt1w_lab_camera_rays_pos_host) -- the start_word with which ray_color continues that sample of a render."""
    p = Context._params(width, height, spp, 0, tile, sample_offset, global_seed, 0, False, strips=strips)
    out = np.empty((p.tile_h, p.tile_w, spp, 8), dtype=np.float64)
    word = np.empty((p.tile_h, p.tile_w, spp), dtype=np.uint32)
    return _twin("rt1w_lab_camera_rays_pos_host", ((scene._h, p, out, word), (out, word)))


def ray_color_host(scene, rays, start_word=None, with_stats=False, **kw):
    """CPU twin of Context.ray_color (librt1w_lab.so: rt1w_lab_ray_color_host, rt_ray_list.h and rt_core.h built for the host): the
    array the GPU must equal bit for bit; with_stats: (array, {"segments": rays traced, "ray_segments": uint32 [n], the rays traced per
    ray of the list (rt1w_lab_ray_color_counts_host)}).  No GPU needed.  This twin says why it refuses a call, as the entries do."""
    args, out = _ray_color_prep(rays, start_word, kw)
    seg = C.c_uint64()
    if not with_stats:
        return _twin("rt1w_lab_ray_color_host", ((scene._h, *args), out), C.byref(seg), says_why=True)
    per_ray = np.zeros(out.shape[0], dtype=np.uint32)
    _twin("rt1w_lab_ray_color_counts_host", ((scene._h, *args), out), C.byref(seg), per_ray, says_why=True)
    return out, {"segments": seg.value, "ray_segments": per_ray}


def path_step_host(scene, states, steps=1, global_seed=0, variant=None, with_stats=False):
    """CPU twin of Context.path_step (librt1w_lab.so: rt1w_lab_path_step_host, rt_path_state.h and rt_core.h built for the host): the
    (states, nodes) the GPU must equal bit for bit; with_stats: + {"segments": levels that traced a ray}.  No GPU needed.  This twin says
    why it refuses a call, as the entries do."""
    args, out = _path_step_prep(states, steps, global_seed, variant)
    seg = C.c_uint64()
    _twin("rt1w_lab_path_step_host", ((scene._h, *args), out), C.byref(seg), says_why=True)
    return out + ({"segments": seg.value},) if with_stats else out


def path_begin_host(scene, width, height, pixels, global_seed=0, max_depth=50):
    """CPU twin of Context.path_begin (librt1w_lab.so: rt1w_lab_path_begin_host) over the scene's own camera.  No GPU needed."""
    args, out = _path_begin_prep(width, height, pixels, global_seed, max_depth)
    return _twin("rt1w_lab_path_begin_host", ((scene._h, *args), out), says_why=True)


def guides_merge_tiles_host(gacc, tile_sums, spp, tile, tiles):
    """CPU twin of Context.guides_merge_tiles (librt1w_lab.so: rt1w_lab_guides_merge_tiles_host)."""
    return _twin("rt1w_lab_guides_merge_tiles_host", _guides_merge_prep(gacc, tile_sums, spp, tile, tiles))


def guides_resolve_host(gacc):
    """CPU twin of Context.guides_resolve (rt1w_lab_guides_resolve_host): the feature buffers [h, w, 8]."""
    return _twin("rt1w_lab_guides_resolve_host", _guides_resolve_prep(gacc))


def temporal_host(cur_frame, cur_aov, cur_cam, prev_hist, prev_len, prev_aov, prev_cam, with_record=False, **kw):
    """CPU twin of Context.temporal_accumulate (librt1w_lab.so: rt1w_lab_temporal_host, the same rt_temporal.h built for the host):
    the (hist, len, frame_out) the GPU must equal bit for bit.  No GPU needed.  with_record: also the tests' record [h, w, 8] of every
    pixel -- fx, fy, the four taps' weights (0 where a tap is not valid), their sum, 1 / 0 history."""
    return _temporal_twin("rt1w_lab_temporal_host", _temporal_prep(cur_frame, cur_aov, cur_cam, prev_hist, None, prev_len, prev_aov, prev_cam, kw),
                          with_record)


def temporal_moments_host(cur_frame, cur_aov, cur_cam, prev_hist, prev_m2, prev_len, prev_aov, prev_cam, with_record=False, **kw):
    """CPU twin of Context.temporal_moments (librt1w_lab.so: rt1w_lab_temporal_moments_host): the (hist, m2, len, frame_out) the GPU must
    equal bit for bit.  No GPU needed.  with_record: also temporal_host's record [h, w, 8]."""
    return _temporal_twin("rt1w_lab_temporal_moments_host",
                          _temporal_prep(cur_frame, cur_aov, cur_cam, prev_hist, prev_m2, prev_len, prev_aov, prev_cam, kw), with_record)


def _temporal_twin(name, prep, with_record):
    rec = np.zeros(prep[1][0].shape[:2] + (8,)) if with_record else None
    out = _twin(name, prep, rec)
    return out + (rec,) if with_record else out


def temporal_variance_host(hist, m2, length, aov):
    """CPU twin of Context.temporal_variance (librt1w_lab.so: rt1w_lab_temporal_variance_host): the var [h, w] the GPU must equal bit
    for bit.  No GPU needed."""
    return _twin("rt1w_lab_temporal_variance_host", _temporal_variance_prep(hist, m2, length, aov))


def scene_set_camera_host(scene, look_from, look_at, vup, vfov_deg, aspect_ratio, aperture, focus_dist, time0, time1):
    """Diagnostics (librt1w_lab.so: rt1w_lab_scene_set_camera): what Context.set_camera does to a context's view, done to a COMMITTED
    scene's own camera record, so that the CPU twins and Scene.flat -- which build their view from the scene -- render the camera a
    live context would.  Everything made from the scene afterwards, a context too, sees a scene committed with these arguments;
    contexts made before keep the camera they copied."""
    _call_lab("rt1w_lab_scene_set_camera", scene._h, _v3(look_from), _v3(look_at), _v3(vup), vfov_deg, aspect_ratio, aperture, focus_dist, time0, time1)


def scene_camera_host(scene):
    """The Camera of a scene's own record (librt1w_lab.so: rt1w_lab_scene_get_camera)."""
    cam = Camera()
    _call_lab("rt1w_lab_scene_get_camera", scene._h, cam)
    return cam


def denoise_host(frame, aov, **kw):
    """CPU twin of Context.denoise (librt1w_lab.so: rt1w_lab_denoise_host, the same rt_denoise.h built for the host): the array the
    GPU must equal bit for bit.  No GPU needed."""
    return _twin("rt1w_lab_denoise_host", _denoise_prep(frame, aov, kw))


def batch_variance_host(sums, aov, batch_spp, keep_albedo=False):
    """CPU twin of Context.batch_variance (librt1w_lab.so: rt1w_lab_batch_variance_host, rt_denoise_var.h built for the host): the
    (frame, var) the GPU must equal bit for bit.  No GPU needed."""
    return _twin("rt1w_lab_batch_variance_host", _batch_variance_prep(sums, aov, batch_spp, keep_albedo))


def denoise_var_host(frame, aov, var, sigma_variance=0.0, **kw):
    """CPU twin of Context.denoise_var (librt1w_lab.so: rt1w_lab_denoise_var_host): the array the GPU must equal bit for bit."""
    return _twin("rt1w_lab_denoise_var_host", _denoise_var_prep(frame, aov, var, sigma_variance, kw))


def accum_merge_host(acc, tile_sums, aov, batch_spp, x0=0, y0=0, keep_albedo=False):
    """CPU twin of Context.accum_merge (librt1w_lab.so: rt1w_lab_accum_merge_host): the accumulator the GPU must equal bit for bit."""
    return _twin("rt1w_lab_accum_merge_host", _merge_prep(acc, tile_sums, aov, batch_spp, x0, y0, keep_albedo))


def accum_merge_tiles_host(acc, tile_sums, aov, batch_spp, tile, tiles, keep_albedo=False):
    """CPU twin of Context.accum_merge_tiles (librt1w_lab.so: rt1w_lab_accum_merge_tiles_host)."""
    return _twin("rt1w_lab_accum_merge_tiles_host", _merge_tiles_prep(acc, tile_sums, aov, batch_spp, tile, tiles, keep_albedo))


def accum_resolve_host(acc, batch_spp):
    """CPU twin of Context.accum_resolve (rt1w_lab_accum_resolve_host): (frame, var, spp)."""
    return _twin("rt1w_lab_accum_resolve_host", _accum_resolve_prep(acc, batch_spp))


def tile_error_host(acc, tile):
    """CPU twin of Context.accum_tile_error (rt1w_lab_tile_error_host)."""
    return _twin("rt1w_lab_tile_error_host", _tile_error_prep(_accum_of(acc), tile))


def halves_resolve_host(acc_a, acc_b, batch_spp):
    """CPU twin of Context.halves_resolve (rt1w_lab_halves_resolve_host): (frame, var, half_a, half_b, spp)."""
    return _twin("rt1w_lab_halves_resolve_host", _halves_resolve_prep(acc_a, acc_b, batch_spp))


def denoise_var_halves_host(frame, aov, var, half_a, half_b, sigma_variance=0.0, with_halves=False, **kw):
    """CPU twin of Context.denoise_var_halves (rt1w_lab_denoise_var_halves_host): (out, err_px), what the GPU must equal bit for bit;
    with_halves: (out, err_px, a', b'), the two filtered halves with the albedo back."""
    prep = _halves_filter_prep(frame, aov, var, half_a, half_b, sigma_variance, kw)
    halves = (np.empty_like(prep[1][0]), np.empty_like(prep[1][0])) if with_halves else (None, None)
    out = _twin("rt1w_lab_denoise_var_halves_host", prep, *halves)
    return out + halves if with_halves else out


def denoise_cross_host(frame, aov, var, half_a, half_b, sigma_variance=0.0, with_record=False, **kw):
    """CPU twin of Context.denoise_cross (rt1w_lab_denoise_cross_host): (out, err_px), what the GPU must equal bit for bit; with_record:
    (out, err_px, rec [h, w, 10]), the last level's record before the finish -- a' rgb, la', va', b' rgb, lb', vb', still demodulated."""
    prep = _halves_filter_prep(frame, aov, var, half_a, half_b, sigma_variance, kw)
    rec = np.empty(prep[1][0].shape[:2] + (10,)) if with_record else None
    out = _twin("rt1w_lab_denoise_cross_host", prep, rec)
    return out + (rec,) if with_record else out


def tile_error_map_host(err_px, tile):
    """CPU twin of Context.tile_error_map (rt1w_lab_tile_error_map_host)."""
    return _twin("rt1w_lab_tile_error_map_host", _tile_error_prep(_error_map_of(err_px), tile))


def adaptive_select(width, height, err, m_per_tile, **adaptive):
    """One round of the plan of rt1w_render_adaptive (rt1w_adaptive_select; host only, no GPU): the row-major indices of the tiles taken, in
    the order taken.  err, m_per_tile: [tiles_y, tiles_x]; adaptive: the keywords of adaptive_params."""
    a = adaptive_params(**adaptive)
    e = np.ascontiguousarray(err, dtype=np.float64)
    m = np.ascontiguousarray(m_per_tile, dtype=np.uint32)
    if e.ndim != 2 or m.shape != e.shape:
        raise ValueError("err and m_per_tile must be [tiles_y, tiles_x]")
    out = np.zeros(max(e.size, 1), dtype=np.uint32)
    n = _call(_lib.rt1w_adaptive_select, a, e.shape[1], e.shape[0], width, height, e, m, out, e.size, stats=False)
    return [int(t) for t in out[:n]]


class f32_exact:
    """Diagnostics (librt1w_lab.so: rt1w_lab_f32_exact), a context manager: inside it every f32 render of the process runs the f32
    kernels built with 64-bit elementary functions instead of the product's -- the build that equals the CPU twin of the f32 core
    (oracle/oracle_flat_f32.cpp) bit for bit.  Same plan, launch, resolve and stats as any f32 render; generic kernels only."""

    def __enter__(self):
        self._was = load_lab().rt1w_lab_f32_exact(1)
        return self

    def __exit__(self, *exc):
        load_lab().rt1w_lab_f32_exact(self._was)
        return False


F32_ELEMENTARY = ("sin", "cos", "atan2", "acos", "log")


def f32_elementary(name, x, y=None, device=0):
    """Diagnostics (librt1w_lab.so: rt1w_lab_f32_elementary): the device's single-precision function `name` of F32_ELEMENTARY over
    float32 arrays, as the product's f32 kernels call it (atan2: of (x, y) = atan2f(x, y))."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y if y is not None else np.zeros_like(x), dtype=np.float32)
    assert x.shape == y.shape and x.ndim == 1 and x.size > 0
    out = np.empty_like(x)
    _call_lab("rt1w_lab_f32_elementary", device, F32_ELEMENTARY.index(name), x, y, x.size, out)
    return out


F32_DRAWS = ("unit", "range_single", "take_range", "take_unit", "gen_unit", "gen_range", "pm1")


def f32_draws(name, words, lo=0.0, hi=1.0, device=0):
    """Diagnostics (librt1w_lab.so: rt1w_lab_f32_draws): the single-precision builds' conversion `name` of F32_DRAWS of 64-bit generator
    words into float32 -- "unit": the unit draw; "range_single": the range draw [lo, hi) with one take and no retry; "take_range" /
    "gen_range": the retrying range draws over a stream of the word and then the word 0 (so a rejected word comes back as lo);
    "take_unit" / "gen_unit": the unit draw's other two spellings; "pm1": the samplers' (-1, 1).  device 0: the host build (no GPU);
    1: one lane per word on GPU 0."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    assert w.ndim == 1 and w.size > 0
    out = np.empty(w.shape, dtype=np.float32)
    _call_lab("rt1w_lab_f32_draws", device, F32_DRAWS.index(name), w, lo, hi, w.size, out)
    return out


DENOISE_ELEMENTARY = ("falloff", "powi")


def denoise_elementary(name, x, e=None, device=0):
    """Diagnostics (librt1w_lab.so: rt1w_lab_denoise_elementary): the function `name` of DENOISE_ELEMENTARY of csrc/rt_denoise.h over a
    float64 array -- rt_dn_falloff(x), or rt_dn_powi(x, e) with uint32 exponents e.  device 0: the host build (no GPU); 1: a kernel on
    GPU 0."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.ndim == 1 and x.size > 0
    if e is not None:
        e = np.ascontiguousarray(np.broadcast_to(np.asarray(e, dtype=np.uint32), x.shape))
    out = np.empty_like(x)
    _call_lab("rt1w_lab_denoise_elementary", device, DENOISE_ELEMENTARY.index(name), x, e, x.size, out)
    return out


def resolve(sums, spp):
    s = np.ascontiguousarray(sums, dtype=np.float64)
    out = np.empty_like(s)
    _call(_lib.rt1w_resolve, s, s.size // 3, spp, out, stats=False)
    return out


def quantize(means):
    m = np.ascontiguousarray(means, dtype=np.float64)
    out = np.empty(m.shape, dtype=np.uint8)
    _call(_lib.rt1w_quantize, m, m.size, out, stats=False)
    return out


def format_ppm(means):
    """P3 text exactly as the reference prints it (src/main.rs:953,1003-1007); means[j, i, 3], row 0 = j = 0."""
    m = np.ascontiguousarray(means, dtype=np.float64)
    h, w = m.shape[:2]
    n = _call(_lib.rt1w_format_ppm, m, w, h, None, 0, stats=False)
    buf = C.create_string_buffer(n + 1)
    _call(_lib.rt1w_format_ppm, m, w, h, buf, n + 1, stats=False)
    return buf.raw[:n].decode()
