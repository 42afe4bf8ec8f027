"""ctypes binding of libsignerf_hip.so (the C ABI declared in include/signerf_hip.h).

There is NO CPU fallback: if the library is missing or a call fails this module raises.
"""

from __future__ import annotations

import ctypes as C
import os
import threading
from typing import NamedTuple, Optional, Tuple

SN_MAX_LEVELS = 16
SN_MAX_PROPOSALS = 2
SN_OK, SN_ERR_INVALID, SN_ERR_HIP, SN_ERR_STATE, SN_ERR_WORKSPACE = 0, 1, 2, 3, 4
SN_ABI_VERSION = 6   # include/signerf_hip.h "ABI evolution": load() refuses a library built with another one
SN_MLP_MAX_LAYERS, SN_MLP_MAX_DIM = 4, 64
SN_MLP_PRECISION_FP32, SN_MLP_PRECISION_FP16 = 0, 1
SN_ADAM_MAX_TENSORS = 32

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# SIGNERF_HIP_LIB: load another build of the library (A/B experiments with tools/ab_lib.sh); the default is the in-tree build
LIB_PATH = os.environ.get("SIGNERF_HIP_LIB") or os.path.join(_PKG_DIR, "libsignerf_hip.so")


class SnHashMlpDesc(C.Structure):
    _fields_ = [
        ("num_levels", C.c_int32),
        ("features_per_level", C.c_int32),
        ("log2_hashmap_size", C.c_int32),
        ("hidden_dim", C.c_int32),
        ("num_layers", C.c_int32),
        ("out_dim", C.c_int32),
        ("scalings", C.c_float * SN_MAX_LEVELS),
        ("grid_mode", C.c_int32),
    ]


class _Sized(C.Structure):
    """A versioned struct of the C ABI: its first field is `struct_size` = sizeof(the struct) in THIS binding's layout, which the library uses
    to read (or write) no more than the binding knows (include/signerf_hip.h "ABI evolution").  Set at construction."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(self)


class SnFieldDesc(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("main_field", SnHashMlpDesc),
        ("geo_feat_dim", C.c_int32),
        ("hidden_dim_color", C.c_int32),
        ("appearance_embed_dim", C.c_int32),
        ("sh_levels", C.c_int32),
        ("sh_remap", C.c_int32),
        ("num_proposals", C.c_int32),
        ("proposals", SnHashMlpDesc * SN_MAX_PROPOSALS),
        ("average_init_density", C.c_float),
        ("histogram_padding", C.c_float),
        ("disable_scene_contraction", C.c_int32),
        ("aabb", C.c_float * 6),
        ("dense_levels", C.c_int32),
        ("dense_copy_cap_mb", C.c_int32),
        ("half_grid", C.c_int32),
    ]


class SnRenderOpts(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("num_proposal_iterations", C.c_int32),
        ("num_proposal_samples", C.c_int32 * SN_MAX_PROPOSALS),
        ("num_nerf_samples", C.c_int32),
        ("near_plane", C.c_float),
        ("far_plane", C.c_float),
        ("chunk_rays", C.c_int32),
        ("precision", C.c_int32),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t),
        ("initial_spacing_bins", C.c_void_p),
        ("pdf_u", C.c_void_p * SN_MAX_PROPOSALS),
        ("background_mode", C.c_int32),
        ("background_rgb", C.c_float * 3),
        ("spacing_mode", C.c_int32),
        ("march_stats", C.c_void_p),
        ("reuse_final_bins", C.c_int32),
    ]


class SnCameraDesc(C.Structure):
    _fields_ = [
        ("c2w", C.c_float * 12),
        ("fx", C.c_float),
        ("fy", C.c_float),
        ("cx", C.c_float),
        ("cy", C.c_float),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("camera_type", C.c_int32),
        ("has_distortion", C.c_int32),
        ("distortion", C.c_float * 6),
    ]


class SnMaskOpts(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("inverse_mask", C.c_int32),
        ("dilate_w", C.c_int32),
        ("dilate_h", C.c_int32),
        ("has_manual_depth", C.c_int32),
        ("manual_min", C.c_double),
        ("manual_max", C.c_double),
        ("additional_depth_radius", C.c_float),
    ]


class SnDebugDump(C.Structure):
    _fields_ = [
        ("main_fetch", C.c_void_p),
        ("main_q", C.c_void_p),
        ("median_index", C.c_void_p),
        ("prop_fetch", C.c_void_p * SN_MAX_PROPOSALS),
        ("prop_q", C.c_void_p * SN_MAX_PROPOSALS),
        ("pdf_index", C.c_void_p * SN_MAX_PROPOSALS),
    ]


class SnDebugLayout(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_dense", C.c_int32),
        ("n_bc", C.c_int32),
        ("dense_res", C.c_uint32 * 12),
        ("dense_off", C.c_uint32 * 12),
        ("dense_bytes", C.c_uint64),
        ("pair_base", C.c_uint32 * SN_MAX_LEVELS),
        ("pair_bytes", C.c_uint64),
        ("feature_scale", C.c_float),
        ("table_bytes", C.c_uint64),
        ("handle_bytes", C.c_uint64),
        ("half_grid_bytes", C.c_uint64),
    ]


class Header(NamedTuple):
    """One public header of the C ABI and what this binding knows of it.  REGISTRY lists them in the order load() checks them;
    tests/test_cabi.py holds every entry against its header file, the library's exports and the version the library reports."""

    key: str             # "core", "mesh", ..., "optim"
    file: str            # the file name under include/
    version_fn: str      # the entry point that answers the header's version
    version_macro: str   # its macro in the header (named in load()'s error text)
    version: int         # the value load() expects the library to report
    functions: dict      # name -> (restype, argtypes): every symbol the header declares
    # True for the entry points tests/golden/handle_free_launches.json was recorded for.  The headers from hashgrid on are newer than
    # the library that recording was made from; what their entry points refuse is swept by their own host tests instead.
    recorded: bool


REGISTRY: Tuple[Header, ...] = ()
# Headers that ship with the package, under signerf_amd/include/ (EXTENSION_DIR): REGISTRY is the tree's include/, file for file
# (tests/test_cabi.py holds the two against each other), and an extension's header stands outside both.  load() binds and version-checks
# either kind; header(key) finds either; functions() stays REGISTRY's.  Each extension has a host test of its own.
EXTENSIONS: Tuple[Header, ...] = ()
EXTENSION_DIR = os.path.join(_PKG_DIR, "include")


def _add(key: str, version: int, recorded: bool, functions: dict, extension: bool = False) -> None:
    global REGISTRY, EXTENSIONS
    infix = "" if key == "core" else "_" + key
    h = Header(key, f"signerf_hip{infix}.h", f"sn{infix}_abi_version", f"SN{infix.upper()}_ABI_VERSION", version, functions, recorded)
    if extension:
        EXTENSIONS += (h,)
    else:
        REGISTRY += (h,)


def header(key: str) -> Header:
    return {h.key: h for h in REGISTRY + EXTENSIONS}[key]


def functions(recorded: Optional[bool] = None) -> dict:
    """name -> (restype, argtypes) over every header, or over the headers whose ``recorded`` flag equals the argument."""
    return {name: sig for h in REGISTRY if recorded is None or h.recorded == recorded for name, sig in h.functions.items()}


_FP = C.c_void_p  # device pointer
# include/signerf_hip.h: the handle, rendering and the stages around it (its host test: tests/test_cabi.py)
_add("core", version=SN_ABI_VERSION, recorded=True, functions={
    "sn_abi_version": (C.c_int, []),
    "sn_create": (C.c_int, [C.POINTER(SnFieldDesc), C.POINTER(C.c_void_p)]),
    "sn_destroy": (C.c_int, [C.c_void_p]),
    "sn_last_error": (C.c_char_p, [C.c_void_p]),
    "sn_upload_weights": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sn_finalize_weights": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sn_generate_rays": (C.c_int, [C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32,
                                   _FP, _FP, _FP, _FP, C.POINTER(C.c_float), _FP, _FP, C.c_void_p]),
    "sn_generate_rays_camera": (C.c_int, [C.POINTER(SnCameraDesc), _FP, C.c_int64, _FP, _FP, _FP, _FP, C.POINTER(C.c_float), _FP, _FP,
                                          C.c_void_p]),
    "sn_intersect_with_aabb": (C.c_int, [_FP, _FP, C.c_int64, C.POINTER(C.c_float), _FP, _FP, C.c_void_p]),
    "sn_intersect_obb": (C.c_int, [_FP, _FP, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float), _FP, _FP, C.c_void_p]),
    "sn_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SnRenderOpts)]),
    "sn_render_rays": (C.c_int, [C.c_void_p, _FP, _FP, _FP, _FP, C.c_int32, C.c_int32, C.POINTER(SnRenderOpts),
                                 _FP, _FP, _FP, _FP, _FP, _FP, C.c_void_p]),
    "sn_render_rays_debug": (C.c_int, [C.c_void_p, _FP, _FP, _FP, _FP, C.c_int32, C.c_int32, C.POINTER(SnRenderOpts),
                                       _FP, _FP, _FP, _FP, _FP, _FP, C.POINTER(SnDebugDump), C.c_void_p]),
    "sn_debug_layout": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(SnDebugLayout)]),
    "sn_debug_read": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _FP, C.c_size_t, C.c_void_p]),
    "sn_debug_reload_env": (C.c_int, [C.c_void_p]),
    "sn_debug_sample_positions": (C.c_int, [_FP, _FP, _FP, _FP, C.c_int64, _FP, _FP, _FP, C.c_void_p]),
    "sn_clock_probe": (C.c_int, [_FP, C.c_double, C.c_void_p]),
    "sn_effective_precision": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "sn_render_normals": (C.c_int, [C.c_void_p, _FP, _FP, _FP, _FP, C.c_int32, C.c_int32, C.POINTER(SnRenderOpts), _FP, _FP, C.c_void_p]),
    "sn_hash_encode": (C.c_int, [C.c_void_p, C.c_int32, _FP, C.c_int64, _FP, _FP, C.c_void_p]),
    "sn_field_forward": (C.c_int, [C.c_void_p, C.c_int32, _FP, _FP, C.c_int64, C.c_int32, _FP, _FP, C.c_void_p]),
    "sn_field_forward_geo": (C.c_int, [C.c_void_p, C.c_int32, _FP, _FP, C.c_int64, C.c_int32, _FP, _FP, _FP, C.c_void_p]),
    "sn_composite": (C.c_int, [_FP, _FP, _FP, C.c_int64, C.c_int32, _FP, _FP, _FP, _FP, _FP, _FP, C.c_void_p]),
    "sn_pdf_sample": (C.c_int, [_FP, _FP, C.c_int64, C.c_int32, C.c_int32, _FP, C.c_float, _FP, _FP, C.c_void_p]),
    "sn_tensor_to_uint8": (C.c_int, [_FP, C.c_int64, _FP, C.c_void_p]),
    "sn_resize_bilinear": (C.c_int, [_FP, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _FP, C.c_int32, C.c_int32, C.c_int64,
                                      C.c_int32, C.c_void_p]),
    "sn_mask_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "sn_aabb_mask_condition": (C.c_int, [_FP, _FP, _FP, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(SnMaskOpts), _FP, _FP,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
})


class SnMeshRasterOpts(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("znear", C.c_float),
        ("zfar", C.c_float),
        ("cull_back_faces", C.c_int32),
    ]


# include/signerf_hip_mesh.h: "shape" masking mode (its host test: tests/test_mesh_host.py)
_add("mesh", version=1, recorded=True, functions={
    "sn_mesh_abi_version": (C.c_int, []),
    "sn_mesh_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "sn_mesh_raster_depth": (C.c_int, [_FP, C.c_int64, _FP, C.c_int64, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float,
                                       C.c_int32, C.c_int32, C.POINTER(SnMeshRasterOpts), _FP, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sn_shape_mask_condition": (C.c_int, [_FP, _FP, C.c_int32, C.c_int32, C.POINTER(SnMaskOpts), _FP, _FP, C.c_void_p, C.c_size_t,
                                          C.c_void_p]),
})



class SnMeshShadeOpts(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base_color", C.c_float * 4),
        ("ambient", C.c_float * 3),
        ("background", C.c_float * 3),
        ("gamma", C.c_int32),
    ]


# include/signerf_hip_mesh_color.h: the mesh's colour image, aabb mode with combine_shape_with_depth (its host test: tests/test_mesh_color_host.py)
_add("mesh_color", version=1, recorded=True, functions={
    "sn_mesh_color_abi_version": (C.c_int, []),
    "sn_mesh_color_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "sn_mesh_raster_color": (C.c_int, [_FP, C.c_int64, _FP, _FP, C.c_int64, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float,
                                       C.c_int32, C.c_int32, C.POINTER(SnMeshRasterOpts), C.POINTER(SnMeshShadeOpts), _FP, _FP, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "sn_aabb_mask_condition_combined": (C.c_int, [_FP, _FP, _FP, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(SnMaskOpts), _FP, _FP,
                                                  _FP, _FP, C.c_void_p, C.c_size_t, C.c_void_p]),
})


class SnMeshRaysOpts(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("znear", C.c_float),
        ("zfar", C.c_float),
        ("cull_back_faces", C.c_int32),
    ]


# include/signerf_hip_mesh_rays.h: the mesh along the camera's own rays (its host test: tests/test_mesh_rays_host.py)
_add("mesh_rays", version=1, recorded=True, functions={
    "sn_mesh_rays_abi_version": (C.c_int, []),
    "sn_mesh_accel_bytes": (C.c_size_t, [C.c_int64]),
    "sn_mesh_cast_rays": (C.c_int, [_FP, _FP, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_void_p, C.c_size_t, _FP, C.c_int64, _FP,
                                    C.c_int64, C.POINTER(SnMeshRaysOpts), C.POINTER(SnMeshShadeOpts), _FP, _FP, C.c_void_p]),
})


class SnMeshMaterial(C.Structure):
    """The frozen 32-byte material record (the kernels read it from device memory)."""

    _fields_ = [
        ("base_color", C.c_float * 4),
        ("texel_offset", C.c_uint32),
        ("tex_width", C.c_int32),
        ("tex_height", C.c_int32),
        ("reserved", C.c_uint32),
    ]


class SnMeshMaterials(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_materials", C.c_int32),
        ("materials", C.c_void_p),
        ("host_materials", C.POINTER(SnMeshMaterial)),
        ("triangle_material", C.c_void_p),
        ("corner_uv", C.c_void_p),
        ("texels", C.c_void_p),
        ("texel_bytes", C.c_uint64),
        ("texture_srgb", C.c_int32),
        ("reserved", C.c_int32),
    ]


# include/signerf_hip_mesh_material.h: the mesh's colour image shaded with its .mtl materials (its host test: tests/test_mesh_material_host.py)
_add("mesh_material", version=1, recorded=True, functions={
    "sn_mesh_material_abi_version": (C.c_int, []),
    "sn_mesh_raster_color_materials": (C.c_int, [_FP, C.c_int64, C.POINTER(SnMeshMaterials), _FP, C.c_int64, C.POINTER(C.c_float), C.c_float,
                                                 C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.POINTER(SnMeshRasterOpts),
                                                 C.POINTER(SnMeshShadeOpts), _FP, _FP, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sn_mesh_cast_rays_materials": (C.c_int, [_FP, _FP, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_void_p, C.c_size_t, _FP, C.c_int64,
                                              C.POINTER(SnMeshMaterials), C.c_int64, C.POINTER(SnMeshRaysOpts), C.POINTER(SnMeshShadeOpts), _FP,
                                              _FP, C.c_void_p]),
})

# include/signerf_hip_ray_batch.h: rays of many cameras in one launch (its host test: tests/test_ray_batch_host.py)
_add("ray_batch", version=1, recorded=True, functions={
    "sn_ray_batch_abi_version": (C.c_int, []),
    "sn_generate_ray_batch": (C.c_int, [_FP, C.c_int32, _FP, _FP, _FP, C.c_int64, _FP, _FP, _FP, _FP, C.POINTER(C.c_float), _FP, _FP, _FP,
                                        C.c_int32, C.c_int32, C.c_int32, _FP, C.c_void_p]),
})

# include/signerf_hip_png.h: a device uint8 image to the bytes of its .png file (its host test: tests/test_png_codes_host.py)
_add("png", version=1, recorded=True, functions={
    "sn_png_abi_version": (C.c_int, []),
    "sn_png_segment_bytes": (C.c_size_t, []),
    "sn_png_max_file_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "sn_png_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "sn_png_encode": (C.c_int, [_FP, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, _FP, C.c_size_t, _FP, C.c_void_p]),
})

# include/signerf_hip_losses.h: differentiable compositing and the sampler losses (its host test: tests/test_losses_host.py)
_add("losses", version=1, recorded=True, functions={
    "sn_losses_abi_version": (C.c_int, []),
    "sn_loss_composite_forward": (C.c_int, [_FP, _FP, _FP, _FP, C.c_int64, C.c_int32, _FP, _FP, _FP, C.c_void_p]),
    "sn_loss_composite_backward": (C.c_int, [_FP, _FP, _FP, _FP, C.c_int64, C.c_int32, _FP, _FP, _FP, _FP, _FP, C.c_void_p]),
    "sn_loss_distortion_forward": (C.c_int, [_FP, _FP, C.c_int64, C.c_int32, _FP, C.c_void_p]),
    "sn_loss_distortion_backward": (C.c_int, [_FP, _FP, _FP, C.c_int64, C.c_int32, _FP, C.c_void_p]),
    "sn_loss_interlevel_forward": (C.c_int, [_FP, _FP, _FP, _FP, C.c_int64, C.c_int32, C.c_int32, _FP, _FP, C.c_void_p]),
    "sn_loss_interlevel_backward": (C.c_int, [_FP, _FP, _FP, _FP, _FP, C.c_int64, C.c_int32, C.c_int32, _FP, C.c_void_p]),
})

# include/signerf_hip_hashgrid.h: the trainable hash grid (its host test: tests/test_hashgrid_host.py)
_add("hashgrid", version=1, recorded=False, functions={
    "sn_hashgrid_abi_version": (C.c_int, []),
    "sn_hashgrid_debug_reload_env": (C.c_int, []),
    "sn_hashgrid_forward": (C.c_int, [_FP, _FP, _FP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, C.c_void_p]),
    "sn_hashgrid_backward": (C.c_int, [_FP, _FP, _FP, _FP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, C.c_void_p]),
})

# signerf_amd/include/signerf_hip_hashgrid_tcnn.h: the trainable tiny-cuda-nn grid (its host test: tests/test_tcnn_hashgrid_host.py)
_add("hashgrid_tcnn", version=1, recorded=False, extension=True, functions={
    "sn_hashgrid_tcnn_abi_version": (C.c_int, []),
    "sn_hashgrid_tcnn_levels": (C.c_int, [C.POINTER(C.c_float), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32)]),
    "sn_hashgrid_tcnn_forward": (C.c_int, [_FP, _FP, _FP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, C.c_void_p]),
    "sn_hashgrid_tcnn_backward": (C.c_int, [_FP, _FP, _FP, _FP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, C.c_void_p]),
})

# signerf_amd/include/signerf_hip_hashgrid_ordered.h: the ordered table gradient of both grids (its host test: tests/test_hashgrid_ordered_host.py)
_add("hashgrid_ordered", version=1, recorded=False, extension=True, functions={
    "sn_hashgrid_ordered_abi_version": (C.c_int, []),
    "sn_hashgrid_ordered_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "sn_hashgrid_ordered_backward": (C.c_int, [_FP, _FP, _FP, _FP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, C.c_void_p, C.c_size_t,
                                               C.c_void_p]),
    "sn_hashgrid_ordered_tcnn_backward": (C.c_int, [_FP, _FP, _FP, _FP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, C.c_void_p, C.c_size_t,
                                                    C.c_void_p]),
})


class SnSamplerRays(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_samples", C.c_int32),
        ("n_rays", C.c_int64),
        ("origins", C.c_void_p),
        ("directions", C.c_void_p),
        ("nears", C.c_void_p),
        ("fars", C.c_void_p),
        ("near_plane", C.c_float),
        ("far_plane", C.c_float),
        ("spacing_mode", C.c_int32),
        ("single_jitter", C.c_int32),
        ("rand", C.c_void_p),
        ("seed", C.c_uint64),
        ("offset", C.c_uint64),
        ("spacing_bins", C.c_void_p),
        ("euclid_bins", C.c_void_p),
        ("deltas", C.c_void_p),
        ("positions", C.c_void_p),
        ("q", C.c_void_p),
        ("selector", C.c_void_p),
        ("rand_out", C.c_void_p),
    ]


class SnSamplerPdf(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_in", C.c_int32),
        ("spacing_bins", C.c_void_p),
        ("weights", C.c_void_p),
        ("u_grid", C.c_void_p),
        ("anneal", C.c_float),
        ("histogram_padding", C.c_float),
    ]


# include/signerf_hip_sampler.h: training-mode proposal sampling (its host test: tests/test_sampler_host.py)
_add("sampler", version=1, recorded=False, functions={
    "sn_sampler_abi_version": (C.c_int, []),
    "sn_sampler_initial": (C.c_int, [C.POINTER(SnSamplerRays), _FP, C.c_void_p]),
    "sn_sampler_pdf": (C.c_int, [C.POINTER(SnSamplerRays), C.POINTER(SnSamplerPdf), C.c_void_p]),
})


class SnMlpDesc(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_layers", C.c_int32),
        ("dims", C.c_int32 * (SN_MLP_MAX_LAYERS + 1)),
        ("precision", C.c_int32),      # SN_MLP_PRECISION_FP32 / _FP16 (the slot "reserved" had: same offset, same size)
        ("weights", C.c_void_p * SN_MLP_MAX_LAYERS),
        ("biases", C.c_void_p * SN_MLP_MAX_LAYERS),
        ("grad_weights", C.c_void_p * SN_MLP_MAX_LAYERS),
        ("grad_biases", C.c_void_p * SN_MLP_MAX_LAYERS),
    ]


# include/signerf_hip_mlp.h: the trainable MLP (its host test: tests/test_mlp_host.py)
_add("mlp", version=1, recorded=False, functions={
    "sn_mlp_abi_version": (C.c_int, []),
    "sn_mlp_forward": (C.c_int, [C.POINTER(SnMlpDesc), _FP, C.c_int64, _FP, C.c_void_p]),
    "sn_mlp_backward_workspace_bytes": (C.c_size_t, [C.POINTER(SnMlpDesc), C.c_int64]),
    "sn_mlp_backward": (C.c_int, [C.POINTER(SnMlpDesc), _FP, _FP, C.c_int64, _FP, C.c_void_p, C.c_size_t, C.c_void_p]),
})

# include/signerf_hip_train_normals.h: analytic normals of training samples (its host test: tests/test_train_normals_host.py)
_add("train_normals", version=1, recorded=False, functions={
    "sn_train_normals_abi_version": (C.c_int, []),
    "sn_train_normals_analytic": (C.c_int, [_FP, _FP, _FP, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SnMlpDesc), _FP, _FP, C.c_void_p]),
})

# include/signerf_hip_normal_losses.h: the per-ray normal terms of a training step (its host test: tests/test_train_normals_host.py)
_add("normal_losses", version=1, recorded=False, functions={
    "sn_normal_losses_abi_version": (C.c_int, []),
    "sn_loss_normals_forward": (C.c_int, [_FP, _FP, _FP, _FP, C.c_int64, C.c_int32, _FP, _FP, _FP, _FP, C.c_void_p]),
    "sn_loss_normals_backward": (C.c_int, [_FP, _FP, _FP, C.c_int64, C.c_int32, _FP, C.c_void_p]),
})



class SnAdamTensor(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("param", C.c_void_p),
        ("grad", C.c_void_p),
        ("exp_avg", C.c_void_p),
        ("exp_avg_sq", C.c_void_p),
        ("step", C.c_void_p),
        ("n", C.c_int64),
        ("group", C.c_int32),
    ]


class SnAdamGroup(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("lr", C.c_float),
        ("beta1", C.c_float),
        ("beta2", C.c_float),
        ("eps", C.c_float),
        ("weight_decay", C.c_float),
        ("max_norm", C.c_float),
    ]


class SnAdamRecord(C.Structure):
    """What the head of sn_adam_step's workspace holds per tensor after the call (a diagnostic)."""

    _fields_ = [
        ("skip", C.c_uint32),
        ("grad_multiplier", C.c_float),
        ("step_size", C.c_float),
        ("sqrt_bc2", C.c_float),
        ("grad_norm", C.c_double),
    ]


# include/signerf_hip_optim.h: the fused Adam step (its host test: tests/test_optim_host.py)
_add("optim", version=1, recorded=False, functions={
    "sn_optim_abi_version": (C.c_int, []),
    "sn_adam_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "sn_adam_step": (C.c_int, [C.POINTER(SnAdamTensor), C.c_int32, C.POINTER(SnAdamGroup), C.c_int32, _FP, _FP, C.c_void_p, C.c_size_t,
                               C.c_void_p]),
})

_lib: Optional[C.CDLL] = None
_lock = threading.Lock()


class SignerfHipError(RuntimeError):
    """Raised when the HIP library is missing or one of its entry points reports an error."""


def load() -> C.CDLL:
    """Loads libsignerf_hip.so (once).  Imports torch first so the process shares ONE HIP runtime."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        import torch  # noqa: F401  (loads torch/lib/libamdhip64.so before our library resolves it)

        if not os.path.exists(LIB_PATH):
            raise SignerfHipError(
                f"{LIB_PATH} not found: build it with `python -m signerf_amd.build` (there is no CPU fallback)")
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise SignerfHipError(f"cannot load {LIB_PATH}: {e}") from e
        bound = dict(functions(), **{name: sig for h in EXTENSIONS for name, sig in h.functions.items()})
        for name, (res, args) in bound.items():
            fn = getattr(lib, name, None)
            if fn is None:
                raise SignerfHipError(f"{LIB_PATH} does not export {name}: it was built from another include/signerf_hip.h -- rebuild it "
                                      "(`python -m signerf_amd.build --force`)")
            fn.restype = res
            fn.argtypes = args
        for h in REGISTRY + EXTENSIONS:
            got = getattr(lib, h.version_fn)()
            if got != h.version:
                raise SignerfHipError(f"{LIB_PATH} reports {h.version_macro} {got}, this binding was written for {h.version}: "
                                      "rebuild the library")
        _lib = lib
        return lib


def check(status: int, handle=None, what: str = "") -> None:
    if status != 0:
        lib = load()
        msg = lib.sn_last_error(handle)
        raise SignerfHipError(f"{what} failed (status {status}): {msg.decode() if msg else ''}")


def ptr(t) -> Optional[int]:
    """Raw device pointer of a CUDA(HIP) fp32/int32 torch tensor (None passes NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise SignerfHipError("tensor must live on the GPU (there is no CPU path)")
    if not t.is_contiguous():
        raise SignerfHipError("tensor must be contiguous")
    return t.data_ptr()


def typed(x, name: str, takes: str) -> None:
    """Raises TypeError unless ``x`` is an fp32 tensor; ``takes`` is the calling module's remark on what its kernels take."""
    import torch

    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: a torch.Tensor expected, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise TypeError(f"{name}: fp32 expected, got {x.dtype} ({takes})")


def prep(x, name: str, takes: str):
    """``typed``, then the device check; returns ``x`` contiguous."""
    typed(x, name, takes)
    if not x.is_cuda:
        raise SignerfHipError(f"{name} must live on the GPU (there is no CPU path)")
    return x.contiguous()


def current_stream() -> int:
    import torch

    return torch.cuda.current_stream().cuda_stream
