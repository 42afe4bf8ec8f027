"""Shape masking mode, CPU side: the OBJ reader, the object pose, the float64 reference rasteriser on analytic scenes, the companion C
header (include/signerf_hip_mesh.h) against the binding and the library's exports, and the generator config.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import mesh_oracle as mo
from abi_helpers import c99_probe, refusal_sweep
from signerf_amd import _lib
from signerf_amd.renderer import RendererConfig, load_obj, model_view, object_pose


# ---- load_obj ------------------------------------------------------------------------------------------------------------------------
def _write(tmp_path, text, name="m.obj"):
    p = tmp_path / name
    p.write_text(text)
    return p


def test_obj_all_face_forms_and_ignored_records(tmp_path):
    p = _write(tmp_path, """# a comment
mtllib m.mtl
o thing
g group
s 1
v 0 0 0
v 1 0 0 0.5 0.5 0.5
v 1 1 0
v 0 1 0   # trailing comment
vt 0 0
vt 1 0
vn 0 0 1
usemtl red
f 1 2 3
f 1/1 3/2 4/1
f 1//1 2//1 4//1
f 2/1/1 3/2/1 4/1/1
f -4 -3 -2
""")
    v, f = load_obj(p)
    assert v.dtype == np.float32 and v.shape == (4, 3) and f.dtype == np.int32
    np.testing.assert_array_equal(v[1], [1, 0, 0])   # vertex colour dropped
    np.testing.assert_array_equal(f, [[0, 1, 2], [0, 2, 3], [0, 1, 3], [1, 2, 3], [0, 1, 2]])


def test_obj_polygon_is_a_triangle_fan(tmp_path):
    p = _write(tmp_path, "v 0 0 0\nv 1 0 0\nv 2 1 0\nv 1 2 0\nv 0 1 0\nf 1 2 3 4 5\n")
    _, f = load_obj(p)
    np.testing.assert_array_equal(f, [[0, 1, 2], [0, 2, 3], [0, 3, 4]])


@pytest.mark.parametrize("text,word", [
    ("v 0 0 0\nv 1 0 0\nf 1 2 3\n", "outside"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", "index 0"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf -4 1 2\n", "outside"),
    ("v 0 0\n", "three coordinates"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n", "three corners"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf a b c\n", "bad face corner"),
    ("v 0 0 0\n", "no faces"),
])
def test_obj_errors_are_clear(tmp_path, text, word):
    with pytest.raises(ValueError, match=word):
        load_obj(_write(tmp_path, text))


def test_obj_missing_or_not_obj(tmp_path):
    with pytest.raises(FileNotFoundError):
        load_obj(tmp_path / "none.obj")
    with pytest.raises(ValueError, match="not an .obj"):
        load_obj(_write(tmp_path, "v 0 0 0\n", "m.ply"))


# ---- pose ----------------------------------------------------------------------------------------------------------------------------
def test_object_pose_closed_forms():
    p = object_pose(RendererConfig(position=[1.0, 2.0, 3.0], rotation=[90, 0, 0], scale=[0.1, 0.2, 0.3]))
    want = np.array([[1, 0, 0, 1], [0, 0, -3, 2], [0, 2, 0, 3], [0, 0, 0, 1]], dtype=np.float64)
    np.testing.assert_allclose(p, want, atol=1e-12)
    p = object_pose(RendererConfig(rotation=[0, 0, 90], scale=[0.1, 0.1, 0.1]))
    np.testing.assert_allclose(p[:3, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-12)
    p = object_pose(RendererConfig(rotation=[0, 90, 0], scale=[0.1, 0.1, 0.1]))
    np.testing.assert_allclose(p[:3, :3], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-12)
    # order: Rz . Ry . Rx
    a = object_pose(RendererConfig(rotation=[30, 45, 60], scale=[0.1, 0.1, 0.1]))[:3, :3]
    rx = object_pose(RendererConfig(rotation=[30, 0, 0], scale=[0.1, 0.1, 0.1]))[:3, :3]
    ry = object_pose(RendererConfig(rotation=[0, 45, 0], scale=[0.1, 0.1, 0.1]))[:3, :3]
    rz = object_pose(RendererConfig(rotation=[0, 0, 60], scale=[0.1, 0.1, 0.1]))[:3, :3]
    np.testing.assert_allclose(a, rz @ ry @ rx, atol=1e-12)
    np.testing.assert_allclose(a @ a.T, np.eye(3), atol=1e-12)


def test_model_view_is_the_full_inverse():
    pose = object_pose(RendererConfig(position=[0.1, -0.2, 0.3], rotation=[10, 20, 30]))
    c2w = np.array([[0, 0, 1, 2.0], [1, 0, 0, -1.0], [0, 1, 0, 0.5]]) * np.array([[1.0], [1.0], [1.0]])
    c2w[:, :3] *= 1.5   # a scaled pose: a transpose would be wrong
    m = np.vstack([c2w, [0, 0, 0, 1]])
    np.testing.assert_allclose(model_view(c2w, pose), (np.linalg.inv(m) @ pose)[:3], atol=1e-12)
    x = np.array([0.3, 0.1, -0.2, 1.0])
    np.testing.assert_allclose(m @ np.append(model_view(c2w, pose) @ x, 1.0), pose @ x, atol=1e-12)


# ---- the reference rasteriser on analytic scenes ------------------------------------------------------------------------------------
H, W, F = 48, 64, 50.0
EYE = np.hstack([np.eye(3), np.zeros((3, 1))])


def _raster(v, f, cull=True, mv=EYE, **kw):
    return mo.raster_depth(v, f, mv, F, F, W / 2, H / 2, H, W, cull=cull, **kw)


def test_oracle_fronto_parallel_quad():
    v, f = mo.quad(-0.51, 0.51, -0.27, 0.27, -2.0)
    d, amb, gr = _raster(v, f)
    want = np.zeros((H, W))
    want[17:31, 19:45] = 2.0    # centres (j + 0.5 - 32) / 25 in [-0.51, 0.51], (i + 0.5 - 24) / 25 in [-0.27, 0.27]
    np.testing.assert_array_equal(d, want)
    assert not gr.any() and amb.sum() <= 4 and (d[amb] == 2.0).all()   # (centres near the shared diagonal: covered either way)


def test_oracle_back_face_culled_or_kept():
    v, f = mo.quad(-0.51, 0.51, -0.27, 0.27, -2.0, ccw_towards=-1)
    assert not _raster(v, f, cull=True)[0].any()
    assert (_raster(v, f, cull=False)[0][17:31, 19:45] == 2.0).all()


def test_oracle_tilted_plane():
    v = np.array([[-1, -1, -2 - 0.3], [1, -1, -2 + 0.3], [1, 1, -2 + 0.3], [-1, 1, -2 - 0.3]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    d, amb, _ = _raster(v, f)
    j = np.arange(W)
    dx = (j + 0.5 - W / 2) / F
    t = 2.0 / (1.0 + 0.3 * dx)        # -t = -2 + 0.3 * (t * dx)
    cov = d > 0
    assert cov.sum() > 0.5 * H * W
    np.testing.assert_allclose(d[cov], np.broadcast_to(t, (H, W))[cov], rtol=1e-6)   # (fp32 vertices)


def test_oracle_near_and_far_clipping():
    v, f = mo.quad(-1, 1, -1, 1, -5e-5)      # closer than znear
    assert not _raster(v, f)[0].any()
    v, f = mo.quad(-10, 10, -10, 10, -11.0)  # beyond zfar
    assert not _raster(v, f)[0].any()
    # a plane sloping through zfar: kept up to t = 10, cut behind
    v = np.array([[-40, -40, -9.0 - 20], [40, -40, -9.0 + 20], [40, 40, -9.0 + 20], [-40, 40, -9.0 - 20]], dtype=np.float32)  # (crosses the camera plane)
    d, amb, _ = _raster(v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))
    cov = d > 0
    assert cov.any() and (~cov).any() and d.max() <= 10.0
    j = np.arange(W)
    t = 9.0 / (1.0 + 0.5 * (j + 0.5 - W / 2) / F)
    full = np.broadcast_to(t, (H, W))
    assert (cov[~amb] == (full[~amb] <= 10.0)).all()


def _brute(tri, fx, fy, cx, cy, h, w):
    """Per-pixel ray / triangle intersection by barycentric coordinates (Moller-Trumbore), an independent float64 check."""
    out = np.zeros((h, w))
    a, b, c = (np.asarray(p, dtype=np.float64) for p in tri)
    for i in range(h):
        for j in range(w):
            d = np.array([(j + 0.5 - cx) / fx, -(i + 0.5 - cy) / fy, -1.0])
            e1, e2 = b - a, c - a
            p = np.cross(d, e2)
            det = e1 @ p
            if abs(det) < 1e-15:
                continue
            s = -a
            u = (s @ p) / det
            q = np.cross(s, e1)
            v = (d @ q) / det
            t = (e2 @ q) / det
            if u >= 0 and v >= 0 and u + v <= 1 and 1e-4 <= t <= 10:
                out[i, j] = t
    return out


def test_oracle_triangle_with_a_vertex_behind_the_camera():
    tri = [[-0.3, -0.2, -1.0], [0.6, -0.1, -1.5], [0.1, 0.4, 1.0]]   # the third vertex is behind the camera
    v = np.asarray(tri, dtype=np.float32)
    for f in ([[0, 1, 2]], [[0, 2, 1]]):
        d, amb, _ = _raster(v, np.asarray(f, dtype=np.int32), cull=False)
        ref = _brute(v, F, F, W / 2, H / 2, H, W)
        assert (d > 0).sum() > 100
        assert ((d > 0) == (ref > 0))[~amb].all()
        np.testing.assert_allclose(d[~amb], ref[~amb], rtol=1e-9)


def test_oracle_random_soup_against_brute_force():
    v, f = mo.triangle_soup(6, seed=3)
    d, amb, _ = _raster(v, f, cull=False)
    ref = np.zeros((H, W))
    for k in range(f.shape[0]):
        r = _brute(v[f[k]], F, F, W / 2, H / 2, H, W)
        ref = np.where((r > 0) & ((ref == 0) | (r < ref)), r, ref)
    assert ((d > 0) == (ref > 0))[~amb].all()
    np.testing.assert_allclose(d[~amb], ref[~amb], rtol=1e-9)


# ---- the companion C header ------------------------------------------------------------------------------------------------------------
def test_mesh_header_binding_and_exports_agree(built_lib):
    """(The header against the binding and the exports: tests/test_cabi.py, for every header.)"""
    lib = _lib.load()
    assert lib.sn_mesh_abi_version() == _lib.header("mesh").version == 1
    blob = open(built_lib, "rb").read()
    assert b"sn_mesh_tile_kernel" in blob and b"sn_shape_condition_kernel" in blob


def test_mesh_opts_layout_matches_c(tmp_path):
    got = [int(x) for x in c99_probe(tmp_path, "signerf_hip_mesh.h", "%zu %zu %zu %zu %zu %d",
                                     "sizeof(SnMeshRasterOpts), offsetof(SnMeshRasterOpts, struct_size), offsetof(SnMeshRasterOpts, znear), "
                                     "offsetof(SnMeshRasterOpts, zfar), offsetof(SnMeshRasterOpts, cull_back_faces), SN_MESH_ABI_VERSION")]
    o = _lib.SnMeshRasterOpts
    assert got == [C.sizeof(o), o.struct_size.offset, o.znear.offset, o.zfar.offset, o.cull_back_faces.offset, _lib.header("mesh").version]
    assert _lib.SnMeshRasterOpts().struct_size == C.sizeof(o)


_NULL_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
fake = 0x1000   # never dereferenced: every call below is refused before the device is touched
mv = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
def opts(size=None, znear=1e-4, zfar=10.0):
    o = _lib.SnMeshRasterOpts(); o.znear, o.zfar = znear, zfar
    if size is not None: o.struct_size = size
    return C.byref(o)
m = _lib.SnMaskOpts()
m0 = _lib.SnMaskOpts()
m0.struct_size = 0   # (set after construction: the constructor fills it in)
calls = {
 "sn_mesh_abi_version": lambda: lib.sn_mesh_abi_version(),
 "sn_mesh_workspace_bytes": lambda: lib.sn_mesh_workspace_bytes(-1, 0, 0),
 "sn_mesh_workspace_bytes_big": lambda: lib.sn_mesh_workspace_bytes(10, 16385, 4),
 "sn_mesh_raster_depth": lambda: lib.sn_mesh_raster_depth(N, 3, N, 1, None, 1.0, 1.0, 0.0, 0.0, 4, 4, None, N, N, 0, N),
 "sn_mesh_raster_depth_no_mesh": lambda: lib.sn_mesh_raster_depth(N, 0, N, 1, mv, 1.0, 1.0, 0.0, 0.0, 4, 4, opts(), fake, fake, 1 << 20, N),
 "sn_mesh_raster_depth_size0": lambda: lib.sn_mesh_raster_depth(fake, 3, fake, 1, mv, 1.0, 1.0, 0.0, 0.0, 4, 4, opts(0), fake, fake, 1 << 20, N),
 "sn_mesh_raster_depth_newer": lambda: lib.sn_mesh_raster_depth(fake, 3, fake, 1, mv, 1.0, 1.0, 0.0, 0.0, 4, 4, opts(64), fake, fake, 1 << 20, N),
 "sn_mesh_raster_depth_znear": lambda: lib.sn_mesh_raster_depth(fake, 3, fake, 1, mv, 1.0, 1.0, 0.0, 0.0, 4, 4, opts(znear=0.0), fake, fake, 1 << 20, N),
 "sn_mesh_raster_depth_fx": lambda: lib.sn_mesh_raster_depth(fake, 3, fake, 1, mv, 0.0, 1.0, 0.0, 0.0, 4, 4, opts(), fake, fake, 1 << 20, N),
 "sn_mesh_raster_depth_ws": lambda: lib.sn_mesh_raster_depth(fake, 3, fake, 1, mv, 1.0, 1.0, 0.0, 0.0, 4, 4, opts(), fake, N, 0, N),
 "sn_shape_mask_condition": lambda: lib.sn_shape_mask_condition(N, N, 4, 4, None, N, N, N, 0, N),
 "sn_shape_mask_condition_opts": lambda: lib.sn_shape_mask_condition(fake, fake, 4, 4, C.byref(m0), fake, N, fake, 1 << 20, N),
 "sn_shape_mask_condition_ws": lambda: lib.sn_shape_mask_condition(fake, fake, 4, 4, C.byref(m), fake, N, N, 0, N),
}
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_mesh_entry_points_refuse_bad_arguments_before_the_device(built_lib):
    """NULL pointers, unset / too-new struct_size, bad planes / intrinsics, no workspace: refused with a status (size queries: 0) in a
    child process -- a crash would be a segfault, not an exception."""
    got = refusal_sweep(_NULL_SWEEP)
    want = {"sn_mesh_abi_version": "1", "sn_mesh_workspace_bytes": "0", "sn_mesh_workspace_bytes_big": "0", "sn_mesh_raster_depth": "1",
            "sn_mesh_raster_depth_no_mesh": "1", "sn_mesh_raster_depth_size0": "1", "sn_mesh_raster_depth_newer": "1",
            "sn_mesh_raster_depth_znear": "1", "sn_mesh_raster_depth_fx": "1", "sn_mesh_raster_depth_ws": "4", "sn_shape_mask_condition": "1",
            "sn_shape_mask_condition_opts": "1", "sn_shape_mask_condition_ws": "4"}
    assert got == want


def test_mesh_workspace_depends_on_the_triangle_count_only(built_lib):
    lib = _lib.load()
    a = lib.sn_mesh_workspace_bytes(1000, 64, 64)
    assert a == lib.sn_mesh_workspace_bytes(1000, 800, 800) and a >= 1000 * 72
    assert lib.sn_mesh_workspace_bytes(0, 8, 8) > 0


# ---- the generator config ------------------------------------------------------------------------------------------------------------
_AABB_KEYS = ["aabb_max", "aabb_min", "additional_depth_radius", "border_width_between_images", "cols", "combine_shape_with_depth", "cx", "cy",
              "dataset_name", "downscale_factor", "fx", "fy", "height", "inverse_mask", "manual_depth", "mask_dialation", "masking_mode", "path",
              "rows", "width"]


def test_aabb_config_yml_is_unchanged_and_shape_mode_records_the_mesh(tmp_path):
    import yaml

    from signerf_amd.datasetgenerator import DatasetGenerator, DatasetGeneratorConfig

    cfg = DatasetGeneratorConfig(path=tmp_path, dataset_name="a", width=8, height=8)
    g = DatasetGenerator(cfg, device="cpu", write_images=False)
    assert g.renderer is None
    g.init_directory()
    text = (tmp_path / "a" / "config.yml").read_text()
    assert sorted(yaml.safe_load(text)) == _AABB_KEYS and "renderer" not in text
    g.dataset.close()

    cfg = DatasetGeneratorConfig(path=tmp_path, dataset_name="s", width=8, height=8, masking_mode="shape",
                                 renderer=RendererConfig(object_path="proxy.obj", position=[0.0, 0.1, 0.0]))
    g = DatasetGenerator(cfg, device="cpu", write_images=False)
    assert g.renderer is not None and g.renderer.object_path == "proxy.obj"
    g.init_directory()
    y = yaml.safe_load((tmp_path / "s" / "config.yml").read_text())
    assert y["masking_mode"] == "shape" and y["renderer"]["object_path"] == "proxy.obj" and y["renderer"]["position"] == [0.0, 0.1, 0.0]
    g.dataset.close()
    # None means the reference's defaults (the bunny at the origin)
    g = DatasetGenerator(DatasetGeneratorConfig(path=tmp_path, dataset_name="d", masking_mode="shape"), device="cpu")
    assert g.renderer.config == RendererConfig() and g.renderer.config.scale == [0.1, 0.1, 0.1]
    assert math.isclose(object_pose(g.renderer.config)[0, 0], 1.0)


def test_shape_mode_without_a_renderer_raises():
    import torch

    from signerf_amd import datasetgenerator as dg

    class _Graph:
        render_aabb = None

        def eval(self):
            pass

        def train(self):
            pass

        def get_outputs_for_camera_ray_bundle(self, b):
            return {"rgb": torch.zeros(2, 2, 3), "depth": torch.ones(2, 2, 1)}

    class _Cam:
        def generate_rays(self, camera_indices, aabb_box):
            return None

    orig = dg._adopt
    dg._adopt = lambda c: c
    try:
        with pytest.raises(ValueError, match="Renderer is None"):
            dg.render_camera(dg.DatasetGeneratorConfig(masking_mode="shape"), _Graph(), _Cam())
    finally:
        dg._adopt = orig
