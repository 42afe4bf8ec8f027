"""Records tests/golden/handle_free_launches.json:  python tests/golden/record_handle_free.py <libsignerf_hip.so of the reference commit>

What an entry point that takes no SnHandle refuses, with which text, and what it launches otherwise -- kernels, grids, blocks, LDS bytes and
parameter blocks -- is host logic; the device only runs what it is handed.  So the reference library -- the commit named in PARENT below,
built as a variant (signerf_amd.build.build(out_path=...)), unchanged -- is run here with its HIP runtime calls served by hip_host_stub.c
(stub_host.py boots it, as for record_launch_variants.py): device memory is one host arena, kernels do nothing and are logged.  Every call of
CALLS goes through that library's own entry point.  Kept per call, in the order of CALLS: the return code, the sn_last_error(NULL) text of a
refused call, and the ordered launches, each "<index into kernels> <grid> <block> <LDS bytes> <SHA-256 of its arguments>", the arguments with every
pointer into the arena replaced by its offset (the stub does that; every buffer of the caller comes from the arena).  The parameter blocks
the reference zero-fills before it fills them are kept whole; of the four it does not zero-fill (MIRRORS: ctypes mirrors, checked against
the code object's argument sizes) the fields are read from the bytes as they were passed, and the padding between them -- stack garbage,
which beside a 4-byte field can look like a pointer into the arena -- is kept as zero.  A mask step also keeps the three
statistics words of its workspace, set to 0xab bytes before the call and read back from the arena after it.  QUERIES are the size and
version queries, kept with their answers.  STAMPS holds which calls clear the host-side stamp of a workspace (SnRenderOpts.reuse_final_bins): for
each of its calls a handle's sn_render_rays leaves its final bins in the workspace, the call is made on that workspace, and what
sn_render_normals with reuse_final_bins then answers is kept.  torch is not imported: it would bring the real runtime into the process.

Recorded twice, in two processes, with identical files.

    --out FILE   write there instead (tests/test_handle_free_launches_host.py runs this file on the tree's own library and compares)"""
import ctypes as C, hashlib, json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
PARENT = "d16188e20e8039c39d2fdbbcd7692cb75fda51a4"
BUF_BYTES = 1 << 23     # of every buffer "@name"; kernels do not run, only workspace carve-ups and the few memsets must fit
NAN, INF = float("nan"), float("inf")

u32, i32, i64, f32, ptr = C.c_uint32, C.c_int32, C.c_int64, C.c_float, C.c_uint64


class RayGenParams(C.Structure):      # sn_stage.h SnRayGenParams
    _fields_ = [("c2w", f32 * 12), ("fx", f32), ("fy", f32), ("cx", f32), ("cy", f32), ("height", i32), ("width", i32), ("camera_type", i32),
                ("has_distortion", i32), ("dist", f32 * 6), ("coords", ptr), ("n", i64), ("origins", ptr), ("directions", ptr), ("pixel_area", ptr),
                ("directions_norm", ptr), ("has_aabb", i32), ("aabb", f32 * 6), ("nears", ptr), ("fars", ptr)]


class CompositeParams(C.Structure):      # sn_stage.h SnCompositeStageParams
    _fields_ = [("bins", ptr), ("density", ptr), ("rgb_s", ptr), ("n_rays", i64), ("n_samples", i32), ("weights", ptr), ("rgb", ptr), ("depth", ptr),
                ("median_index", ptr), ("acc", ptr), ("exp_raw", ptr), ("minmax", ptr)]


class PdfParams(C.Structure):      # sn_proposal.h SnPdfStageParams
    _fields_ = [("sbins", ptr), ("weights", ptr), ("n_rays", i64), ("n_in", i32), ("n_out", i32), ("u", ptr), ("hist_pad", f32), ("new_bins", ptr),
                ("inds", ptr)]


class ResizeParams(C.Structure):      # sn_mask.h SnResizeParams
    _fields_ = [("src", ptr), ("dst", ptr), ("src_u8", i32), ("src_h", i32), ("src_w", i32), ("dst_h", i32), ("dst_w", i32), ("channels", i32),
                ("src_row_stride", i64), ("dst_row_stride", i64), ("threshold", i32)]


# the parameter blocks the reference fills field by field without zeroing them first, by the kernel's name
MIRRORS = {"sn_generate_rays_kernel": RayGenParams, "sn_composite_kernel": CompositeParams, "sn_pdf_stage_kernel": PdfParams,
           "sn_resize_bilinear_kernel": ResizeParams}

C2W = (1.0, 0.0, 0.0, 0.5, 0.0, 0.8, -0.6, 0.25, 0.0, 0.6, 0.8, -1.5)
AABB = (-1.0, -1.5, -2.0, 1.0, 1.5, 2.0)
MV = (1.0, 0.0, 0.0, 0.1, 0.0, 1.0, 0.0, -0.2, 0.0, 0.0, 1.0, -3.0)
H, W = 17, 33


def S(t, **fields):
    """A struct of _lib, by name, with these fields set (struct_size: overrides what the binding sets)."""
    return dict(fields, _t=t)


def call(fn, *args, add=0):
    """The answer of a size query of the library for the values of the named arguments of this call (or literal numbers), plus `add`."""
    return {"_call": fn, "args": list(args), "add": add}


CAM = S("SnCameraDesc", c2w=C2W, fx=30.0, fy=31.0, cx=16.5, cy=8.5, height=H, width=W, camera_type=1, has_distortion=0,
        distortion=(0.1, -0.05, 0.01, 0.002, 0.003, -0.004))
MASK_OPTS = S("SnMaskOpts", inverse_mask=0, dilate_w=0, dilate_h=0, has_manual_depth=1, manual_min=0.25, manual_max=7.5, additional_depth_radius=0.125)
RASTER_OPTS = S("SnMeshRasterOpts", znear=0.05, zfar=100.0, cull_back_faces=1)
RAYS_OPTS = S("SnMeshRaysOpts", znear=0.05, zfar=100.0, cull_back_faces=1)
SHADE = S("SnMeshShadeOpts", base_color=(0.8, 0.7, 0.6, 1.0), ambient=(0.1, 0.2, 0.3), background=(1.0, 0.5, 0.25), gamma=1)
MAT = [dict(base_color=(0.5, 0.6, 0.7, 1.0), texel_offset=0, tex_width=0, tex_height=0), dict(base_color=(1.0, 1.0, 1.0, 1.0), texel_offset=16, tex_width=8, tex_height=6)]
MATERIALS = S("SnMeshMaterials", n_materials=2, materials="@materials", host_materials=MAT, triangle_material="@triangle_material", corner_uv="@corner_uv",
              texels="@texels", texel_bytes=4 * 64, texture_srgb=1)
RAYS_OUT = [("origins", "@origins"), ("directions", "@directions"), ("pixel_area", "@pixel_area"), ("directions_norm", "@directions_norm"),
            ("aabb", AABB), ("nears", "@nears"), ("fars", "@fars")]
RAYS_IN = [("origins", "@origins"), ("directions", "@directions")]
FRAME = [("height", H), ("width", W)]
MASK_TAIL = [("mask", "@mask"), ("condition", "@condition"), ("workspace", "@ws"), ("workspace_bytes", call("sn_mask_workspace_bytes", "height", "width"))]
MESH = [("vertices", "@vertices"), ("n_vertices", 200)]
TRIS = [("triangles", "@triangles"), ("n_triangles", 300)]
RASTER_CAM = [("model_view", MV), ("fx", 30.0), ("fy", 31.0), ("cx", 16.5), ("cy", 8.5)] + FRAME + [("opts", RASTER_OPTS)]
RASTER_TAIL = [("workspace", "@ws"), ("workspace_bytes", call("sn_mesh_workspace_bytes", "n_triangles", "height", "width"))]
CAST = RAYS_IN + [("height", W), ("width", H), ("forward", (0.0, 0.6, -1.6)), ("accel", "@accel"), ("accel_bytes", call("sn_mesh_accel_bytes", "n_triangles"))] + TRIS
LOSS_TW = [("t", "@t"), ("w", "@w")]
LOSS_ENV = LOSS_TW + [("t_env", "@t_env"), ("w_env", "@w_env")]
LOSS_COMP = [("deltas", "@deltas"), ("density", "@density"), ("colour", "@colour"), ("background", "@background"), ("R", 3), ("S", 1)]

# an accepted call of every entry point: its arguments in order, by name ("@name": that buffer of the arena, "@name+8": 8 bytes into it)
DEFAULTS = {
    "sn_generate_rays": [("c2w", C2W), ("fx", 30.0), ("fy", 31.0), ("cx", 16.5), ("cy", 8.5)] + FRAME + RAYS_OUT,
    "sn_generate_rays_camera": [("cam", CAM), ("coords", None), ("n_coords", 0)] + RAYS_OUT,
    "sn_intersect_with_aabb": RAYS_IN + [("n_rays", 257), ("aabb", AABB), ("nears", "@nears"), ("fars", "@fars")],
    "sn_intersect_obb": RAYS_IN + [("n_rays", 257), ("world2box", MV), ("size", (1.0, 2.5, 3.0)), ("nears", "@nears"), ("fars", "@fars")],
    "sn_debug_sample_positions": RAYS_IN + [("starts", "@starts"), ("ends", "@ends"), ("n", 257), ("q_strict", "@q_strict"), ("q_exact", "@q_exact"),
                                            ("q_fast", "@q_fast")],
    "sn_clock_probe": [("out", "@probe"), ("seconds", 0.25)],
    "sn_composite": [("euclid_bins", "@bins"), ("density", "@density"), ("rgb_samples", "@colour"), ("n_rays", 257), ("n_samples", 5), ("weights", "@weights"),
                     ("rgb", "@rgb"), ("depth", "@depth"), ("median_index", "@median_index"), ("accumulation", "@acc"), ("expected_depth", None)],
    "sn_pdf_sample": [("spacing_bins", "@bins"), ("weights", "@weights"), ("n_rays", 257), ("n_in", 8), ("n_out", 4), ("u", "@u"), ("histogram_padding", 0.01),
                      ("new_bins", "@new_bins"), ("inds", "@inds")],
    "sn_tensor_to_uint8": [("in", "@rgb"), ("n", 257), ("out", "@color")],
    "sn_resize_bilinear": [("src", "@src"), ("src_u8", 0), ("src_h", 5), ("src_w", 7), ("src_row_stride", 21), ("channels", 3), ("dst", "@dst"), ("dst_h", 9),
                           ("dst_w", 11), ("dst_row_stride", 33), ("threshold", 0)],
    "sn_aabb_mask_condition": RAYS_IN + [("depth", "@depth")] + FRAME + [("aabb", AABB), ("opts", MASK_OPTS)] + MASK_TAIL,
    "sn_shape_mask_condition": [("mesh_depth", "@mesh_depth"), ("nerf_depth", "@depth")] + FRAME + [("opts", MASK_OPTS)] + MASK_TAIL,
    "sn_aabb_mask_condition_combined": RAYS_IN + [("depth", "@depth")] + FRAME + [("aabb", AABB), ("opts", MASK_OPTS), ("mesh_depth", "@mesh_depth"),
                                                                                 ("mesh_color", "@mesh_color")] + MASK_TAIL,
    "sn_mesh_raster_depth": MESH + TRIS + RASTER_CAM + [("depth", "@mesh_depth")] + RASTER_TAIL,
    "sn_mesh_raster_color": MESH + [("vertex_colors", "@vertex_colors")] + TRIS + RASTER_CAM + [("shade", SHADE), ("depth", "@mesh_depth"), ("color", "@mesh_color")]
                            + RASTER_TAIL,
    "sn_mesh_raster_color_materials": MESH + [("materials", MATERIALS)] + TRIS + RASTER_CAM + [("shade", SHADE), ("depth", "@mesh_depth"), ("color", "@mesh_color")]
                                      + RASTER_TAIL,
    "sn_mesh_cast_rays": CAST + [("vertex_colors", "@vertex_colors"), ("n_vertices", 200), ("opts", RAYS_OPTS), ("shade", SHADE), ("depth", "@mesh_depth"),
                                 ("color", "@mesh_color")],
    "sn_mesh_cast_rays_materials": CAST + [("materials", MATERIALS), ("n_vertices", 200), ("opts", RAYS_OPTS), ("shade", SHADE), ("depth", "@mesh_depth"),
                                           ("color", "@mesh_color")],
    "sn_generate_ray_batch": [("cameras", "@cameras"), ("n_cameras", 3), ("ray_indices", "@ray_indices"), ("camera_indices", None), ("coords", None), ("n", 257)]
                             + RAYS_OUT + [("images", None), ("img_h", 0), ("img_w", 0), ("img_c", 0), ("pixels", None)],
    "sn_png_encode": [("image", "@color"), ("h", 1), ("w", 1), ("c", 1), ("workspace", "@ws"), ("workspace_bytes", call("sn_png_workspace_bytes", "h", "w", "c")),
                      ("file", "@file"), ("file_capacity", call("sn_png_max_file_bytes", "h", "w", "c")), ("file_bytes", "@file_bytes")],
    "sn_loss_composite_forward": LOSS_COMP + [("weights", "@weights"), ("rgb", "@rgb"), ("accumulation", "@acc")],
    "sn_loss_composite_backward": LOSS_COMP + [("grad_weights", "@grad_weights"), ("grad_rgb", "@grad_rgb"), ("grad_acc", "@grad_acc"),
                                               ("grad_density", "@grad_density"), ("grad_colour", "@grad_colour")],
    "sn_loss_distortion_forward": LOSS_TW + [("R", 3), ("S", 1), ("loss", "@loss")],
    "sn_loss_distortion_backward": LOSS_TW + [("grad_loss", "@grad_loss"), ("R", 3), ("S", 1), ("grad_w", "@grad_w")],
    "sn_loss_interlevel_forward": LOSS_ENV + [("R", 3), ("S", 1), ("P", 1), ("loss", "@loss"), ("w_outer", "@w_outer")],
    "sn_loss_interlevel_backward": LOSS_ENV + [("grad_loss", "@grad_loss"), ("R", 3), ("S", 1), ("P", 1), ("grad_w_env", "@grad_w_env")],
}
MASK_STEPS = ("sn_aabb_mask_condition", "sn_shape_mask_condition", "sn_aabb_mask_condition_combined")
RASTERS = ("sn_mesh_raster_depth", "sn_mesh_raster_color", "sn_mesh_raster_color_materials")
CASTS = ("sn_mesh_cast_rays", "sn_mesh_cast_rays_materials")
LOSSES = [fn for fn in DEFAULTS if fn.startswith("sn_loss_")]


def matrix():
    """[(key, entry point, {argument: value replacing the default}, {environment variable: value during the call})]"""
    out = []

    def add(fn, label, env=None, **over):
        assert not set(over) - {k for k, _ in DEFAULTS[fn]}, (fn, label)
        out.append((f"{fn}: {label}", fn, over, env or {}))

    # ---- accepted --------------------------------------------------------------------------------------------------------------------
    add("sn_generate_rays", "full frame")
    add("sn_generate_rays", "no aabb, no optional outputs", aabb=None, nears=None, fars=None, pixel_area=None, directions_norm=None)
    for ct, dist in ((1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)):      # (3, 1): equirectangular never un-distorts, <3, false>
        add("sn_generate_rays_camera", f"camera_type={ct} distortion={dist}", cam=dict(CAM, camera_type=ct, has_distortion=dist))
    add("sn_generate_rays_camera", "coords", coords="@coords", n_coords=257)
    add("sn_generate_rays_camera", "coords, n == 0", coords="@coords", n_coords=0)
    add("sn_generate_rays_camera", "no coords: n_coords is not looked at", n_coords=-1)
    for fn, n in (("sn_intersect_with_aabb", "n_rays"), ("sn_intersect_obb", "n_rays"), ("sn_debug_sample_positions", "n"), ("sn_composite", "n_rays"),
                  ("sn_pdf_sample", "n_rays"), ("sn_tensor_to_uint8", "n"), ("sn_generate_ray_batch", "n")):
        add(fn, "n = 257")
        add(fn, "n == 0", **{n: 0})
    add("sn_debug_sample_positions", "no outputs", q_strict=None, q_exact=None, q_fast=None)
    add("sn_composite", "expected_depth", expected_depth="@expected_depth")
    add("sn_composite", "expected_depth, no other outputs", expected_depth="@expected_depth", weights=None, rgb=None, depth=None, median_index=None, accumulation=None)
    add("sn_pdf_sample", "largest sizes, no inds", n_in=256, n_out=256, inds=None)
    add("sn_resize_bilinear", "float source")
    add("sn_resize_bilinear", "uint8 source, threshold", src_u8=1, threshold=1, src_row_stride=24, dst_row_stride=40)
    add("sn_clock_probe", "a quarter of a second")
    for fn in MASK_STEPS:
        for kw, kh in ((0, 0), (1, 1), (5, 3)):      # (5, 3): the elliptical element, its rows in the parameter block
            add(fn, f"dilate {kw}x{kh}", opts=dict(MASK_OPTS, dilate_w=kw, dilate_h=kh))
        add(fn, "inverse, automatic depth range, no condition", opts=dict(MASK_OPTS, inverse_mask=1, has_manual_depth=0), condition=None)
    add("sn_aabb_mask_condition", "the shortest SnMaskOpts", opts=dict(MASK_OPTS, struct_size=44))
    add("sn_aabb_mask_condition", "the largest element", opts=dict(MASK_OPTS, dilate_w=256, dilate_h=256))
    for fn in RASTERS:
        add(fn, "300 triangles")
        add(fn, "no triangles", n_triangles=0, vertices=None, triangles=None, n_vertices=0)
        add(fn, "front and back faces", opts=dict(RASTER_OPTS, cull_back_faces=0))
        if fn != "sn_mesh_raster_depth":
            add(fn, "no depth", depth=None)
    add("sn_mesh_raster_color", "no vertex colours, no gamma", vertex_colors=None, shade=dict(SHADE, gamma=0))
    add("sn_mesh_raster_color_materials", "one material, no textures", materials=dict(MATERIALS, n_materials=1, texels=None, texel_bytes=0, corner_uv=None))
    add("sn_mesh_cast_rays", "depth and colour")
    add("sn_mesh_cast_rays", "depth only", color=None, shade=None, triangles=None, vertex_colors=None)
    add("sn_mesh_cast_rays", "no triangles", n_triangles=0)
    add("sn_mesh_cast_rays_materials", "depth and colour")
    add("sn_mesh_cast_rays_materials", "no triangle indices", triangles=None)
    add("sn_generate_ray_batch", "camera_indices and coords", ray_indices=None, camera_indices="@camera_indices", coords="@coords")
    add("sn_generate_ray_batch", "pixel gather", images="@images", img_h=5, img_w=7, img_c=3, pixels="@pixels")
    add("sn_generate_ray_batch", "no aabb", aabb=None, nears=None, fars=None)
    add("sn_png_encode", "1x1 greyscale")
    add("sn_png_encode", "64x100 RGB, two segments", h=64, w=100, c=3)
    for fn in LOSSES:
        big = dict(S=1024, P=1024) if "interlevel" in fn else dict(S=1024)
        add(fn, "R = 3, smallest sizes")
        add(fn, "R = 3, largest sizes", **big)
        add(fn, "R == 0, no pointers", R=0, **{k: None for k, v in DEFAULTS[fn] if isinstance(v, str)})
    add("sn_loss_composite_forward", "weights only, no colour", colour=None, background=None, rgb=None, accumulation=None)
    add("sn_loss_composite_backward", "no colour", colour=None, background=None, grad_rgb=None, grad_colour=None, grad_weights=None)
    add("sn_loss_interlevel_forward", "w_outer only", w=None, loss=None)

    # ---- refused: every argument-dependent refusal, and two faults at once where the order of the checks shows ---------------------------
    def shared(group, keep):
        """add() for the refusals of a helper that the entry points of `group` share: all of them through the first one, of the others
        those of `keep` (the helper builds its texts from the entry point's name; what an entry point checks before it is in `keep`)."""
        return lambda fn, label, **over: add(fn, label, **over) if fn == group[0] or label in keep else None

    add("sn_generate_rays", "c2w NULL", c2w=None)
    add("sn_generate_rays", "width 0", width=0)
    add("sn_generate_rays_camera", "cam NULL", cam=None)
    add("sn_generate_rays_camera", "height 0", cam=dict(CAM, height=0))
    add("sn_generate_rays_camera", "coords with n_coords < 0", coords="@coords", n_coords=-1)
    add("sn_generate_rays_camera", "camera_type 4", cam=dict(CAM, camera_type=4))
    add("sn_generate_rays_camera", "two faults: width 0 and camera_type 0", cam=dict(CAM, width=0, camera_type=0))
    add("sn_intersect_with_aabb", "aabb NULL", aabb=None)
    add("sn_intersect_with_aabb", "n_rays -1", n_rays=-1)
    add("sn_intersect_obb", "size NULL", size=None)
    add("sn_intersect_obb", "n_rays -1", n_rays=-1)
    add("sn_debug_sample_positions", "ends NULL", ends=None)
    add("sn_debug_sample_positions", "n -1", n=-1)
    add("sn_clock_probe", "out NULL", out=None)
    add("sn_clock_probe", "seconds 0", seconds=0.0)
    add("sn_clock_probe", "seconds above 1", seconds=1.5)
    add("sn_clock_probe", "seconds NaN", seconds=NAN)
    add("sn_clock_probe", "no wall-clock rate", env={"HIP_STUB_CUS": "0"})      # (the stub answers every device attribute with it)
    add("sn_composite", "density NULL", density=None)
    add("sn_composite", "n_samples 0", n_samples=0)
    add("sn_composite", "n_rays -1", n_rays=-1)
    add("sn_pdf_sample", "u NULL", u=None)
    add("sn_pdf_sample", "n_in 257", n_in=257)
    add("sn_pdf_sample", "n_out 0", n_out=0)
    add("sn_tensor_to_uint8", "out NULL", out=None)
    add("sn_tensor_to_uint8", "n -1", n=-1)
    add("sn_resize_bilinear", "dst NULL", dst=None)
    add("sn_resize_bilinear", "src_row_stride below a row", src_row_stride=20)
    add("sn_resize_bilinear", "channels 0", channels=0)
    some = shared(MASK_STEPS, {"mask NULL", "struct_size 0", "dilate 3x0", "workspace one byte short", "two faults: mask NULL and struct_size 0"})
    for fn in MASK_STEPS:
        some(fn, "mask NULL", mask=None)
        some(fn, "opts NULL", opts=None)
        some(fn, "height 0", height=0)
        some(fn, "struct_size 0", opts=dict(MASK_OPTS, struct_size=0))
        some(fn, "struct_size below the first layout", opts=dict(MASK_OPTS, struct_size=40))
        some(fn, "struct_size of a newer header", opts=dict(MASK_OPTS, struct_size=56))
        some(fn, "dilate_w 257", opts=dict(MASK_OPTS, dilate_w=257, dilate_h=3))
        some(fn, "dilate_h -1", opts=dict(MASK_OPTS, dilate_w=3, dilate_h=-1))
        some(fn, "dilate 3x0", opts=dict(MASK_OPTS, dilate_w=3, dilate_h=0))
        some(fn, "workspace NULL", workspace=None)
        some(fn, "workspace one byte short", workspace_bytes=call("sn_mask_workspace_bytes", "height", "width", add=-1))
        some(fn, "two faults: mask NULL and struct_size 0", mask=None, opts=dict(MASK_OPTS, struct_size=0))
        some(fn, "two faults: struct_size 0 and workspace NULL", opts=dict(MASK_OPTS, struct_size=0), workspace=None)
        some(fn, "two faults: dilate 3x0 and workspace NULL", opts=dict(MASK_OPTS, dilate_w=3, dilate_h=0), workspace=None)
    add("sn_aabb_mask_condition", "aabb NULL", aabb=None)
    add("sn_shape_mask_condition", "mesh_depth NULL", mesh_depth=None)
    add("sn_aabb_mask_condition_combined", "mesh_color NULL", mesh_color=None)
    bad_shade = dict(SHADE, ambient=(0.1, NAN, 0.3))
    bad_materials = dict(MATERIALS, n_materials=0)
    some = shared(RASTERS, {"model_view NULL", "znear 0", "fx 0", "workspace one byte short", "two faults: znear 0 and fx 0"})
    for fn in RASTERS:
        some(fn, "model_view NULL", model_view=None)
        some(fn, "opts NULL", opts=None)
        some(fn, "n_vertices -1", n_vertices=-1)
        some(fn, "n_triangles -1", n_triangles=-1)
        some(fn, "n_triangles above 2^30", n_triangles=(1 << 30) + 1)
        some(fn, "width 16385", width=16385)
        some(fn, "triangles without vertices", vertices=None)
        some(fn, "triangles without vertices: n_vertices 0", n_vertices=0)
        some(fn, "SnMeshRasterOpts struct_size 0", opts=dict(RASTER_OPTS, struct_size=0))
        some(fn, "SnMeshRasterOpts struct_size of a newer header", opts=dict(RASTER_OPTS, struct_size=20))
        some(fn, "znear 0", opts=dict(RASTER_OPTS, znear=0.0))
        some(fn, "zfar below znear", opts=dict(RASTER_OPTS, zfar=0.01))
        some(fn, "zfar inf", opts=dict(RASTER_OPTS, zfar=INF))
        some(fn, "znear NaN", opts=dict(RASTER_OPTS, znear=NAN))
        some(fn, "fx 0", fx=0.0)
        some(fn, "cy NaN", cy=NAN)
        some(fn, "workspace NULL", workspace=None)
        some(fn, "workspace one byte short", workspace_bytes=call("sn_mesh_workspace_bytes", "n_triangles", "height", "width", add=-1))
        some(fn, "two faults: znear 0 and fx 0", opts=dict(RASTER_OPTS, znear=0.0), fx=0.0)
        some(fn, "two faults: fx 0 and workspace NULL", fx=0.0, workspace=None)
        if fn != "sn_mesh_raster_depth":
            add(fn, "color NULL", color=None)
            add(fn, "shade NULL", shade=None)
            add(fn, "SnMeshShadeOpts struct_size 0", shade=dict(SHADE, struct_size=0))
            add(fn, "SnMeshShadeOpts struct_size of a newer header", shade=dict(SHADE, struct_size=64))
            add(fn, "base_color inf", shade=dict(SHADE, base_color=(0.8, INF, 0.6, 1.0)))
            add(fn, "ambient NaN", shade=bad_shade)
            add(fn, "background NaN", shade=dict(SHADE, background=(NAN, 0.5, 0.25)))
            add(fn, "two faults: ambient NaN and znear 0", shade=bad_shade, opts=dict(RASTER_OPTS, znear=0.0))
            add(fn, "two faults: ambient NaN and workspace NULL", shade=bad_shade, workspace=None)
            add(fn, "two faults: shade NULL and model_view NULL", shade=None, model_view=None)
    add("sn_mesh_raster_depth", "depth NULL", depth=None)
    some = shared(CASTS, {"origins NULL", "shade NULL", "znear 0", "accel not 16-byte aligned", "ambient NaN", "two faults: forward zero and ambient NaN",
                          "two faults: shade NULL and accel not aligned"})
    for fn in CASTS:
        some(fn, "origins NULL", origins=None)
        some(fn, "forward NULL", forward=None)
        some(fn, "depth NULL", depth=None)
        some(fn, "height 16385", height=16385)
        some(fn, "n_triangles above 2^26", n_triangles=(1 << 26) + 1)
        some(fn, "n_vertices -1", n_vertices=-1)
        some(fn, "shade NULL", shade=None)
        some(fn, "SnMeshRaysOpts struct_size 0", opts=dict(RAYS_OPTS, struct_size=0))
        some(fn, "znear 0", opts=dict(RAYS_OPTS, znear=0.0))
        some(fn, "zfar inf", opts=dict(RAYS_OPTS, zfar=INF))
        some(fn, "accel_bytes of another mesh", accel_bytes=call("sn_mesh_accel_bytes", 299))
        some(fn, "accel not 16-byte aligned", accel="@accel+8")
        some(fn, "forward zero", forward=(0.0, 0.0, 0.0))
        some(fn, "forward NaN", forward=(0.0, NAN, 1.0))
        some(fn, "SnMeshShadeOpts struct_size 0", shade=dict(SHADE, struct_size=0))
        some(fn, "ambient NaN", shade=bad_shade)
        some(fn, "two faults: znear 0 and accel not aligned", opts=dict(RAYS_OPTS, znear=0.0), accel="@accel+8")
        some(fn, "two faults: accel not aligned and forward zero", accel="@accel+8", forward=(0.0, 0.0, 0.0))
        some(fn, "two faults: forward zero and ambient NaN", forward=(0.0, 0.0, 0.0), shade=bad_shade)
        some(fn, "two faults: shade NULL and accel not aligned", shade=None, accel="@accel+8")
    add("sn_mesh_cast_rays", "colour without triangle indices", triangles=None)
    add("sn_mesh_cast_rays", "depth only: a bad shade is not looked at", color=None, shade=bad_shade)
    add("sn_mesh_cast_rays_materials", "color NULL", color=None)
    add("sn_mesh_cast_rays_materials", "n_triangles -1", n_triangles=-1)
    WITH_MATERIALS = ("sn_mesh_raster_color_materials", "sn_mesh_cast_rays_materials")
    some = shared(WITH_MATERIALS, {"materials NULL", "n_materials 0", "material 1: base_color NaN", "two faults: n_materials 0 and shade NULL",
                                   "two faults: n_materials 0 and ambient NaN"})
    for fn in WITH_MATERIALS:
        some(fn, "materials NULL", materials=None)
        some(fn, "SnMeshMaterials struct_size 0", materials=dict(MATERIALS, struct_size=0))
        some(fn, "n_materials 0", materials=bad_materials)
        some(fn, "n_materials 65536", materials=dict(MATERIALS, n_materials=65536))
        some(fn, "materials.materials NULL", materials=dict(MATERIALS, materials=None))
        some(fn, "host_materials NULL", materials=dict(MATERIALS, host_materials=None))
        some(fn, "triangle_material NULL", materials=dict(MATERIALS, triangle_material=None))
        some(fn, "materials not 16-byte aligned", materials=dict(MATERIALS, materials="@materials+8"))
        some(fn, "corner_uv not 8-byte aligned", materials=dict(MATERIALS, corner_uv="@corner_uv+4"))
        some(fn, "texels not 4-byte aligned", materials=dict(MATERIALS, texels="@texels+2"))
        some(fn, "texels NULL with texel_bytes", materials=dict(MATERIALS, texels=None))
        some(fn, "material 1: base_color NaN", materials=dict(MATERIALS, host_materials=[MAT[0], dict(MAT[1], base_color=(1.0, NAN, 1.0, 1.0))]))
        some(fn, "material 1: a texture of 0 x 6", materials=dict(MATERIALS, host_materials=[MAT[0], dict(MAT[1], tex_width=0)]))
        some(fn, "material 0: a texture side of 16385", materials=dict(MATERIALS, host_materials=[dict(MAT[0], tex_width=16385, tex_height=1), MAT[1]]))
        some(fn, "material 1: texture beyond the blob", materials=dict(MATERIALS, host_materials=[MAT[0], dict(MAT[1], texel_offset=17)]))
        some(fn, "two faults: n_materials 0 and shade NULL", materials=bad_materials, shade=None)
        some(fn, "two faults: n_materials 0 and ambient NaN", materials=bad_materials, shade=bad_shade)
    add("sn_mesh_raster_color_materials", "two faults: n_materials 0 and znear 0", materials=bad_materials, opts=dict(RASTER_OPTS, znear=0.0))
    add("sn_mesh_raster_color_materials", "two faults: n_triangles -1 and materials NULL", n_triangles=-1, materials=None)
    add("sn_mesh_cast_rays_materials", "two faults: n_materials 0 and accel not aligned", materials=bad_materials, accel="@accel+8")
    add("sn_mesh_cast_rays_materials", "two faults: color NULL and materials NULL", color=None, materials=None)
    pairs = dict(ray_indices=None, camera_indices="@camera_indices", coords="@coords")
    add("sn_generate_ray_batch", "cameras NULL", cameras=None)
    add("sn_generate_ray_batch", "n_cameras 0", n_cameras=0)
    add("sn_generate_ray_batch", "n -1", n=-1)
    add("sn_generate_ray_batch", "both index forms", camera_indices="@camera_indices", coords="@coords")
    add("sn_generate_ray_batch", "no index form", ray_indices=None)
    add("sn_generate_ray_batch", "camera_indices without coords", ray_indices=None, camera_indices="@camera_indices")
    add("sn_generate_ray_batch", "images without pixels", images="@images", img_h=5, img_w=7, img_c=3)
    add("sn_generate_ray_batch", "pixels with camera_indices", images="@images", img_h=5, img_w=7, img_c=3, pixels="@pixels", **pairs)
    add("sn_generate_ray_batch", "img_c 5", images="@images", img_h=5, img_w=7, img_c=5, pixels="@pixels")
    add("sn_generate_ray_batch", "img_h 0", images="@images", img_h=0, img_w=7, img_c=3, pixels="@pixels")
    add("sn_generate_ray_batch", "n beyond the grid", n=(1 << 39) + 1)
    add("sn_generate_ray_batch", "n == 0 with a fault: refused", n=0, ray_indices=None)
    add("sn_generate_ray_batch", "two faults: n -1 and no index form", n=-1, ray_indices=None)
    add("sn_png_encode", "image NULL", image=None)
    add("sn_png_encode", "file_bytes NULL", file_bytes=None)
    add("sn_png_encode", "c 2", c=2)
    add("sn_png_encode", "h 0", h=0)
    add("sn_png_encode", "w 8193", w=8193)
    add("sn_png_encode", "workspace one byte short", workspace_bytes=call("sn_png_workspace_bytes", "h", "w", "c", add=-1))
    add("sn_png_encode", "workspace not 16-byte aligned", workspace="@ws+8")
    add("sn_png_encode", "file_capacity one byte short", file_capacity=call("sn_png_max_file_bytes", "h", "w", "c", add=-1))
    add("sn_png_encode", "two faults: c 2 and h 0", c=2, h=0)
    add("sn_png_encode", "two faults: workspace and file_capacity short", workspace_bytes=0, file_capacity=0)
    for fn in LOSSES:
        first = next(k for k, v in DEFAULTS[fn] if isinstance(v, str))
        add(fn, "R -1", R=-1)
        add(fn, f"{first} NULL", **{first: None})
        add(fn, f"two faults: S 1025 and {first} NULL", S=1025, **{first: None})
        if fn == "sn_loss_interlevel_forward":      # every check of the prologue all six share, through the one that has a P
            add(fn, "S 0", S=0)
            add(fn, "S 1025", S=1025)
            add(fn, "R 2^31", R=1 << 31)
            add(fn, "P 0", P=0)
            add(fn, "P 1025", P=1025)
            add(fn, "two faults: R -1 and S 0", R=-1, S=0)
            add(fn, "two faults: S 0 and P 0", S=0, P=0)
            add(fn, f"two faults: {first} NULL and R 2^31", R=1 << 31, **{first: None})
    add("sn_loss_composite_forward", "no output", weights=None, rgb=None, accumulation=None)
    add("sn_loss_composite_forward", "rgb without colour", colour=None)
    add("sn_loss_composite_backward", "grad_density NULL", grad_density=None)
    add("sn_loss_composite_backward", "grad_colour without colour", colour=None, grad_rgb=None)
    add("sn_loss_distortion_forward", "loss NULL", loss=None)
    add("sn_loss_distortion_backward", "grad_w NULL", grad_w=None)
    add("sn_loss_interlevel_forward", "no output", loss=None, w_outer=None)
    add("sn_loss_interlevel_forward", "loss without w", w=None)
    add("sn_loss_interlevel_backward", "grad_w_env NULL", grad_w_env=None)
    assert len({k for k, *_ in out}) == len(out)
    return out


CALLS = matrix()
# the size and version queries: (entry point, arguments)
QUERIES = [(fn, ()) for fn in ("sn_abi_version", "sn_mesh_abi_version", "sn_mesh_color_abi_version", "sn_mesh_rays_abi_version", "sn_mesh_material_abi_version",
                               "sn_ray_batch_abi_version", "sn_png_abi_version", "sn_losses_abi_version", "sn_png_segment_bytes")]
QUERIES += [("sn_mask_workspace_bytes", a) for a in ((H, W), (1, 1), (0, W), (H, -1))]
QUERIES += [(fn, a) for fn in ("sn_mesh_workspace_bytes", "sn_mesh_color_workspace_bytes")
            for a in ((300, H, W), (0, H, W), (-1, H, W), ((1 << 30) + 1, H, W), (300, 0, W), (300, H, 16385))]
QUERIES += [("sn_mesh_accel_bytes", (n,)) for n in (300, 1, 0, -1, 1 << 26, (1 << 26) + 1)]
QUERIES += [(fn, a) for fn in ("sn_png_max_file_bytes", "sn_png_workspace_bytes") for a in ((1, 1, 1), (64, 100, 3), (8192, 8192, 3), (0, 1, 1), (1, 8193, 3), (1, 1, 2))]


# the calls of CALLS that are handed a workspace, one accepted and two refused of each: does the stamp of that workspace survive them?
STAMPS = [f"{fn}: {label}" for fn in MASK_STEPS for label in ("dilate 0x0", "dilate 3x0", "workspace one byte short")]
STAMPS += [f"{fn}: {label}" for fn in RASTERS for label in ("300 triangles", "fx 0", "workspace one byte short")] + ["sn_png_encode: 1x1 greyscale"]
assert not set(STAMPS) - {key for key, *_ in CALLS}


def buffers():
    """The names of the arena's buffers the matrix uses, sorted: their offsets do not depend on the order of the calls."""
    names = set()

    def walk(v):
        if isinstance(v, str) and v.startswith("@"):
            names.add(v[1:].split("+")[0])
        elif isinstance(v, dict):
            for x in v.values():
                walk(x)
        elif isinstance(v, (list, tuple)):
            for x in v:
                walk(x)

    walk(DEFAULTS)
    walk([over for _, _, over, _ in CALLS])
    return sorted(names | {"normals"})


if __name__ == "__main__":
    lib_path = os.path.abspath(sys.argv[1])
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "handle_free_launches.json")
    import stub_host
    host = stub_host.boot(lib_path)
    _lib, wc, stub, lib, ARGS, dev = host._lib, host.wc, host.stub, host.lib, host.args, host.dev
    KERNELS = sorted(ARGS)

    MIRROR = {}      # kernel -> the mirror of its parameter block
    for name, sizes in ARGS.items():
        for base, mirror in MIRRORS.items():
            if base in name:
                assert sizes == [C.sizeof(mirror)], (name, sizes, C.sizeof(mirror))
                MIRROR[name] = mirror
    assert len(MIRROR) == 8, sorted(MIRROR)      # five instantiations of the ray generator and the three others

    def size_of(kernel):
        (name, sizes), = [(k, v) for k, v in ARGS.items() if kernel in k]
        assert len(sizes) == 1
        return sizes[0]

    # SnMaskParams is zero-filled whole and is a multiple of 8 bytes: the two structs that embed it have no padding behind it, their own
    # fields are pointers that are always set, so their blocks are compared byte for byte
    assert size_of("sn_shape_visible_kernel") == size_of("sn_mask_visible_kernel") + 8 == size_of("sn_shape_condition_kernel")
    assert size_of("sn_mask_condition_combined_kernel") == size_of("sn_mask_visible_kernel") + 16 and size_of("sn_mask_visible_kernel") % 8 == 0

    ARENA = dev(256)      # the arena's first block: no buffer of the caller has offset 0, which a logged parameter block shows as null
    BUF = {name: dev(BUF_BYTES) for name in buffers()}

    def resolve(v, t, named, alive):
        """The ctypes value of a symbolic one, for an argument (or field) of ctypes type t."""
        if isinstance(v, str):
            name, _, off = v[1:].partition("+")
            return BUF[name] + int(off or 0)
        if isinstance(v, dict) and "_call" in v:
            return getattr(lib, v["_call"])(*[named[a] if isinstance(a, str) else a for a in v["args"]]) + v["add"]
        if isinstance(v, dict):
            s = getattr(_lib, v["_t"])()
            types = dict(s._fields_)
            for k, x in v.items():
                if k == "_t":
                    continue
                if isinstance(x, list):      # host_materials: a host array of records
                    arr = (_lib.SnMeshMaterial * len(x))()
                    for rec, fields in zip(arr, x):
                        for fk, fv in fields.items():
                            if isinstance(fv, tuple):
                                for i, e in enumerate(fv):
                                    getattr(rec, fk)[i] = e
                            else:
                                setattr(rec, fk, fv)
                    alive.append(arr)
                    s.host_materials = arr
                elif isinstance(x, tuple):
                    for i, e in enumerate(x):
                        getattr(s, k)[i] = e
                elif k == "host_materials":
                    s.host_materials = None
                else:
                    setattr(s, k, resolve(x, types[k], named, alive) if isinstance(x, str) else x)
            alive.append(s)
            return C.byref(s)
        if isinstance(v, tuple):
            arr = (C.c_float * len(v))(*v)
            alive.append(arr)
            return arr
        return v

    def run(key, fn, over, env):
        spec = [(k, over.get(k, v)) for k, v in DEFAULTS[fn]]
        types = _lib.functions(recorded=True)[fn][1]
        assert len(types) == len(spec) + 1, fn      # (+ the stream)
        named, alive, args = {}, [], []
        for (k, v), t in zip(spec, types):      # plain numbers first: the size queries refer to them by name
            if isinstance(v, (int, float)) and not isinstance(v, bool):
                named[k] = v
        for (k, v), t in zip(spec, types):
            args.append(resolve(v, t, named, alive))
        stats = None
        if fn in MASK_STEPS and named["height"] > 0 and named["width"] > 0 and dict(spec)["workspace"] == "@ws":
            n = named["height"] * named["width"]
            a256 = lambda x: (x + 255) & ~255
            stats = (C.c_uint32 * 3).from_address(BUF["ws"] + a256(n) + a256(named["height"] * (named["width"] + 1) * 4))
            stats[0] = stats[1] = stats[2] = 0xabababab
        os.environ.update(env)
        stub.stub_clear()
        rc = getattr(lib, fn)(*args, None)
        for k in env:
            del os.environ[k]
        launches = []
        for i in range(stub.stub_launches()):
            geom = (C.c_uint64 * 7)()
            stub.stub_launch_geometry(i, geom)
            n = stub.stub_launch_args(i, None, 0)
            buf = (C.c_ubyte * max(n, 1))()
            stub.stub_launch_args(i, buf, n)
            name = stub.stub_launch_name(i).decode()
            assert n > 0 and name in ARGS, name
            block = bytes(buf)[:n]
            if name in MIRROR:      # field by field from the bytes as they were passed: pointers as arena offsets, padding as zero
                p = MIRROR[name]()
                assert stub.stub_launch_raw_args(i, C.byref(p), n) == n == C.sizeof(p)
                q = MIRROR[name]()
                for f, t in p._fields_:
                    v = getattr(p, f)
                    if t is ptr and v:
                        assert ARENA < v < ARENA + (1 << 34), (name, f)
                        v -= ARENA
                    setattr(q, f, v)
                block = bytes(q)
            g = list(geom)
            launches.append(f"{KERNELS.index(name)} {g[0]},{g[1]},{g[2]} {g[3]},{g[4]},{g[5]} {g[6]} {hashlib.sha256(block).hexdigest()[:16]}")
        rec = {"key": key, "rc": rc, "error": lib.sn_last_error(None).decode() if rc else "", "launches": launches}
        if stats is not None:
            rec["stats"] = list(stats)
        return rec

    calls = [run(*c) for c in CALLS]
    queries = [[fn, list(a), getattr(lib, fn)(*a)] for fn, a in QUERIES]

    # ---- the stamps, after every logged call: the handle's buffers come from the arena too ---------------------------------------------
    import numpy as np
    case = wc.cases()["ordinary"]
    stub.stub_set_absmax((C.c_uint32 * 3)(*[int(np.float32(a).view(np.uint32)) for a in case.absmax]))
    desc, h = wc.field_desc(case), C.c_void_p(None)
    assert lib.sn_create(C.byref(desc), C.byref(h)) == 0, lib.sn_last_error(None)
    named = [(n, case.tensors[n]) for n, _ in wc.tensor_names(case.app_dim, case.pred_normals, case.n_prop)]
    named.append(("field.mlp_base.encoder.hash_table", case.table(-1)))
    named += [(f"proposal_networks.{i}.mlp_base.encoder.hash_table", case.table(i)) for i in range(case.n_prop)]
    for n, a in named:
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert lib.sn_upload_weights(h, n.encode(), a.ctypes.data, a.size * 4, None) == 0, (n, lib.sn_last_error(h))
    assert lib.sn_finalize_weights(h, None) == 0, lib.sn_last_error(h)
    o = _lib.SnRenderOpts()
    o.num_proposal_iterations, o.num_nerf_samples, o.near_plane, o.far_plane, o.chunk_rays, o.precision = 2, 48, 0.05, 1000.0, 1 << 15, 1
    o.num_proposal_samples[0], o.num_proposal_samples[1] = 64, 32
    o.workspace, o.workspace_bytes = BUF["ws"], BUF_BYTES
    assert 0 < lib.sn_workspace_bytes(h, H, W, C.byref(o)) <= BUF_BYTES
    rays = (h, BUF["origins"], BUF["directions"], None, None, H, W, C.byref(o))
    stamps = []
    for c in CALLS:
        if c[0] in STAMPS:
            o.reuse_final_bins = 0
            assert lib.sn_render_rays(*rays, BUF["rgb"], BUF["depth"], BUF["acc"], None, None, None, None) == 0, lib.sn_last_error(h)
            rc = run(*c)["rc"]
            o.reuse_final_bins = 1
            rc_reuse = lib.sn_render_normals(*rays, BUF["normals"], None, None)
            stamps.append([c[0], rc, rc_reuse, lib.sn_last_error(h).decode() if rc_reuse else ""])
    lib.sn_destroy(h)
    used = sorted({int(l.split()[0]) for c in calls for l in c["launches"]})       # only the kernels some call launched are listed
    for c in calls:
        c["launches"] = [" ".join([str(used.index(int(l.split()[0])))] + l.split()[1:]) for l in c["launches"]]
    print(len(calls), "calls,", sum(c["rc"] == 0 for c in calls), "accepted,", len(used), "kernels launched", flush=True)
    with open(out_path, "w") as f:      # one line per kernel, query and call
        f.write('{\n "provenance": ' + json.dumps({"parent_commit": PARENT, "procedure": __doc__}) + ',\n "kernels": [\n'
                + ",\n".join("  " + json.dumps(KERNELS[k]) for k in used) + '\n ],\n "queries": [\n' + ",\n".join("  " + json.dumps(q) for q in queries)
                + '\n ],\n "stamps": [\n' + ",\n".join("  " + json.dumps(x) for x in stamps) + '\n ],\n "calls": [\n' + ",\n".join("  " + json.dumps(c) for c in calls) + "\n ]\n}\n")
