"""combine_shape_with_depth, CPU side: the companion C header include/signerf_hip_mesh_color.h against the binding and the library's exports,
its struct layout, its argument checks, the OBJ reader's vertex colours, the colour oracle on an analytic scene and the generator config.
No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mesh_color_oracle as mco
import mesh_oracle as mo
from abi_helpers import c99_probe, refusal_sweep
from helpers import ROOT
from signerf_amd import _lib
from signerf_amd.renderer import RendererConfig, load_obj, shade_defaults

GOLDEN = os.path.join(ROOT, "tests", "golden", "pyrender")


# ---- the companion C header ------------------------------------------------------------------------------------------------------------
def test_mesh_color_header_binding_and_exports_agree(built_lib):
    """(The header against the binding, the exports and build.HEADERS: tests/test_cabi.py, for every header.)"""
    lib = _lib.load()
    assert lib.sn_mesh_color_abi_version() == _lib.header("mesh_color").version == 1
    assert lib.sn_mesh_abi_version() == _lib.header("mesh").version == 1   # the depth header is untouched
    blob = open(built_lib, "rb").read()
    assert b"sn_mesh_tile_color_kernel" in blob and b"sn_mask_condition_combined_kernel" in blob


def test_shade_opts_layout_matches_c(tmp_path):
    got = [int(x) for x in c99_probe(tmp_path, "signerf_hip_mesh_color.h", "%zu %zu %zu %zu %zu %zu %d",
                                     "sizeof(SnMeshShadeOpts), offsetof(SnMeshShadeOpts, struct_size), offsetof(SnMeshShadeOpts, base_color), "
                                     "offsetof(SnMeshShadeOpts, ambient), offsetof(SnMeshShadeOpts, background), "
                                     "offsetof(SnMeshShadeOpts, gamma), SN_MESH_COLOR_ABI_VERSION")]
    o = _lib.SnMeshShadeOpts
    assert got == [C.sizeof(o), o.struct_size.offset, o.base_color.offset, o.ambient.offset, o.background.offset, o.gamma.offset,
                   _lib.header("mesh_color").version]
    assert _lib.SnMeshShadeOpts().struct_size == C.sizeof(o)


_NULL_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
fake = 0x1000   # never dereferenced: every call below is refused before the device is touched
mv = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
box = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
def ropts(size=None, znear=1e-4, zfar=10.0):
    o = _lib.SnMeshRasterOpts(); o.znear, o.zfar = znear, zfar
    if size is not None: o.struct_size = size
    return C.byref(o)
def sopts(size=None, nan=False):
    o = _lib.SnMeshShadeOpts(); o.base_color[:] = [0.3, 0.3, 0.3, 1.0]; o.ambient[:] = [1.0, 1.0, 1.0]; o.background[:] = [1.0, 1.0, 1.0]
    if nan: o.ambient[1] = float("nan")
    if size is not None: o.struct_size = size
    return C.byref(o)
def raster(vc=fake, tris=fake, shade=None, opts=None, color=fake, ws=fake, wsb=1 << 20, fx=1.0, h=4):
    return lib.sn_mesh_raster_color(fake, 3, vc, tris, 1, mv, fx, 1.0, 0.0, 0.0, h, 4, opts if opts is not None else ropts(),
                                    shade if shade is not None else sopts(), fake, color, ws, wsb, N)
m = _lib.SnMaskOpts()
m0 = _lib.SnMaskOpts()
m0.struct_size = 0   # (set after construction: the constructor fills it in)
mbig = _lib.SnMaskOpts()
mbig.dilate_w = 300; mbig.dilate_h = 300
def comb(md=fake, mc=fake, opts=C.byref(m), ws=fake, wsb=1 << 20):
    return lib.sn_aabb_mask_condition_combined(fake, fake, fake, 4, 4, box, opts, md, mc, fake, N, ws, wsb, N)
calls = {
 "sn_mesh_color_abi_version": lambda: lib.sn_mesh_color_abi_version(),
 "sn_mesh_color_workspace_bytes": lambda: lib.sn_mesh_color_workspace_bytes(-1, 0, 0),
 "sn_mesh_color_workspace_bytes_big": lambda: lib.sn_mesh_color_workspace_bytes(10, 16385, 4),
 "sn_mesh_raster_color": lambda: lib.sn_mesh_raster_color(N, 3, N, N, 1, None, 1.0, 1.0, 0.0, 0.0, 4, 4, None, None, N, N, N, 0, N),
 "raster_no_color_out": lambda: raster(color=N),
 "raster_no_tris": lambda: raster(tris=N),
 "raster_no_shade_ptr": lambda: lib.sn_mesh_raster_color(fake, 3, fake, fake, 1, mv, 1.0, 1.0, 0.0, 0.0, 4, 4, ropts(), None, fake, fake, fake, 1 << 20, N),
 "raster_shade_size0": lambda: raster(shade=sopts(0)),
 "raster_shade_newer": lambda: raster(shade=sopts(64)),
 "raster_shade_nan": lambda: raster(shade=sopts(nan=True)),
 "raster_opts_size0": lambda: raster(opts=ropts(0)),
 "raster_znear": lambda: raster(opts=ropts(znear=0.0)),
 "raster_fx": lambda: raster(fx=0.0),
 "raster_height": lambda: raster(h=0),
 "raster_ws": lambda: raster(ws=N, wsb=0),
 "raster_ws_small": lambda: raster(wsb=16),
 "sn_aabb_mask_condition_combined": lambda: lib.sn_aabb_mask_condition_combined(N, N, N, 4, 4, None, None, N, N, N, N, N, 0, N),
 "comb_no_mesh_depth": lambda: comb(md=N),
 "comb_no_mesh_color": lambda: comb(mc=N),
 "comb_opts_size0": lambda: comb(opts=C.byref(m0)),
 "comb_dilation": lambda: comb(opts=C.byref(mbig)),
 "comb_ws": lambda: comb(ws=N, wsb=0),
}
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_mesh_color_entry_points_refuse_bad_arguments_before_the_device(built_lib):
    """NULL pointers, unset / too-new struct_size, non-finite shading, bad planes / intrinsics / sizes, no workspace: refused with a
    status (size queries: 0) in a child process -- a crash would be a segfault, not an exception."""
    got = refusal_sweep(_NULL_SWEEP)
    want = {k: "1" for k in got}
    want.update({"sn_mesh_color_abi_version": "1", "sn_mesh_color_workspace_bytes": "0", "sn_mesh_color_workspace_bytes_big": "0",
                 "raster_ws": "4", "raster_ws_small": "4", "comb_ws": "4"})
    assert len(got) == 22 and got == want


def test_mesh_color_workspace_is_the_depth_workspace(built_lib):
    lib = _lib.load()
    for f, h, w in ((1000, 64, 64), (1000, 800, 800), (0, 8, 8), (70000, 800, 800)):
        assert lib.sn_mesh_color_workspace_bytes(f, h, w) == lib.sn_mesh_workspace_bytes(f, h, w) > 0


# ---- load_obj with colours -------------------------------------------------------------------------------------------------------------
def _write(tmp_path, text, name="m.obj"):
    p = tmp_path / name
    p.write_text(text)
    return p


def test_obj_vertex_colors_parsed(tmp_path):
    p = _write(tmp_path, "v 0 0 0 1 0 0.5\nv 1 0 0 0.2 0.4 0.6\nv 0 1 0 0 0 0   # c\nf 1 2 3\n")
    v, f, c = load_obj(p, with_colors=True)
    assert c.dtype == np.uint8 and c.shape == (3, 4)
    np.testing.assert_array_equal(c, [[255, 0, 128, 255], [51, 102, 153, 255], [0, 0, 0, 255]])   # np.round(c * 255)
    v2, f2 = load_obj(p)   # the default keeps the 2-tuple
    np.testing.assert_array_equal(v, v2)
    np.testing.assert_array_equal(f, f2)
    np.testing.assert_array_equal(v[0], [0, 0, 0])
    p = _write(tmp_path, "v 0 0 0 255 0 12\nv 1 0 0 3 4 5\nv 0 1 0 0 0 0\nf 1 2 3\n", "b.obj")   # 0..255 values
    np.testing.assert_array_equal(load_obj(p, with_colors=True)[2][:, :3], [[255, 0, 12], [3, 4, 5], [0, 0, 0]])


def test_obj_without_colors_gives_none(tmp_path):
    p = _write(tmp_path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    v, f, c = load_obj(p, with_colors=True)
    assert c is None and v.shape == (3, 3) and f.shape == (1, 3)


@pytest.mark.parametrize("text,line", [
    ("v 0 0 0 1 1 1\nv 1 0 0\nv 0 1 0 1 1 1\nf 1 2 3\n", 2),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0 0.5 0.5 0.5\nf 1 2 3\n", 3),
])
def test_obj_partial_colors_raise_with_file_and_line(tmp_path, text, line):
    p = _write(tmp_path, text)
    with pytest.raises(ValueError, match=re.escape(f"{p}:{line}:")):
        load_obj(p, with_colors=True)
    assert len(load_obj(p)) == 2   # the depth-only reader (shape mode) keeps reading such a file, as before


def test_obj_bad_colors_raise(tmp_path):
    with pytest.raises(ValueError, match="bad vertex colour"):
        load_obj(_write(tmp_path, "v 0 0 0 a b c\nv 1 0 0 1 1 1\nv 0 1 0 1 1 1\nf 1 2 3\n"), with_colors=True)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        load_obj(_write(tmp_path, "v 0 0 0 -1 0 0\nv 1 0 0 1 1 1\nv 0 1 0 1 1 1\nf 1 2 3\n", "n.obj"), with_colors=True)


# ---- the shading restatement ---------------------------------------------------------------------------------------------------------
def test_shade_defaults_and_oracle_constants():
    assert shade_defaults(False)["base_color"] == (0.3, 0.3, 0.3, 1.0) and shade_defaults(True)["base_color"] == (1.0, 1.0, 1.0, 1.0)
    assert shade_defaults(False)["ambient"] == (1.0, 1.0, 1.0) and shade_defaults(False)["background"] == (1.0, 1.0, 1.0)
    assert round(255 * 0.3 ** (1 / 2.2)) == 148
    H, W, F = 48, 64, 50.0
    v, f = mo.quad(-0.51, 0.51, -0.27, 0.27, -2.0)
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    tri, depth, bary, gap = mco.raster_front(v, f, eye, F, F, W / 2, H / 2, H, W)
    ref, _, _ = mo.raster_depth(v, f, eye, F, F, W / 2, H / 2, H, W)
    np.testing.assert_array_equal(depth, ref)
    x = mco.shade(tri, bary, f)
    assert set(np.unique(np.floor(x + 0.5))) == {148.0, 255.0}
    # vertex colours: the barycentrics reproduce a corner's colour at that corner and are affine along the plane
    vc = np.array([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255], [255, 255, 255, 255]], np.uint8)
    x = mco.shade(tri, bary, f, vc, base_color=(1, 1, 1, 1), gamma=False)
    cov = tri >= 0
    assert np.allclose(x[cov].sum(-1)[tri[cov] == 0], 255.0)   # red + green + blue weights sum to 1 on triangle 0
    i, j = np.nonzero(cov)
    k = np.argmin(np.hypot(j + 0.5 - 32 - 0.51 * 25, i + 0.5 - 24 - 0.27 * 25))   # the pixel nearest to corner 1 (x1, y0)
    assert x[i[k], j[k], 1] > 200


def test_combined_oracle_reduces_to_the_plain_condition():
    """Mesh behind the NeRF everywhere: the combined restatement is the plain aabb restatement; in front: 1 - colour / 255 there."""
    from oracle import nerfacto as onf
    from oracle import signerf_utils as su
    from signerf_amd import scene

    H = W = 40
    r = onf.generate_rays(scene.benchmark_cameras(8)[1, :3], 56.0, 56.0, W / 2, H / 2, H, W)
    g = torch.Generator().manual_seed(0)
    depth = 2.0 + torch.rand(H, W, 1, generator=g)
    depth[15:25, 15:25] = 0.5
    box = torch.tensor([[-0.1, -0.1, -0.1], [0.1, 0.1, 0.1]])
    color = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    pm, pc = su.aabb_mask_and_condition(depth, r["origins"], r["directions"], box, (5, 5))
    assert pm.any()
    m, c = mco.combined_mask_and_condition(depth, r["origins"], r["directions"], box, depth + 1.0, color, (5, 5))
    assert torch.equal(m, pm) and torch.equal(c, pc)
    front = torch.zeros(H, W, 1)
    front[10:20, 10:20] = 0.1
    m, c = mco.combined_mask_and_condition(depth, r["origins"], r["directions"], box, front, color, (5, 5))
    cv = front > 0
    assert torch.equal(m, pm) and torch.equal(c[~cv], pc[~cv])
    assert torch.equal(c[cv], 1 - color[..., 0:1][cv] / 255.0)


# ---- the generator config ------------------------------------------------------------------------------------------------------------
def test_aabb_combine_config_has_a_renderer_and_records_it(tmp_path):
    import yaml

    from signerf_amd.datasetgenerator import DatasetGenerator, DatasetGeneratorConfig

    cfg = DatasetGeneratorConfig(path=tmp_path, dataset_name="c", width=8, height=8, combine_shape_with_depth=True,
                                 renderer=RendererConfig(object_path="proxy.obj", position=[0.0, 0.1, 0.0]))
    g = DatasetGenerator(cfg, device="cpu", write_images=False)
    assert g.renderer is not None and g.renderer.object_path == "proxy.obj"
    g.init_directory()
    y = yaml.safe_load((tmp_path / "c" / "config.yml").read_text())
    assert y["masking_mode"] == "aabb" and y["combine_shape_with_depth"] is True
    assert y["renderer"]["object_path"] == "proxy.obj" and y["renderer"]["position"] == [0.0, 0.1, 0.0]
    g.dataset.close()
    # None means the reference's defaults; plain aabb keeps no renderer, even with a renderer config
    g = DatasetGenerator(DatasetGeneratorConfig(path=tmp_path, dataset_name="d", combine_shape_with_depth=True), device="cpu")
    assert g.renderer is not None and g.renderer.config == RendererConfig()
    g = DatasetGenerator(DatasetGeneratorConfig(path=tmp_path, dataset_name="e", renderer=RendererConfig()), device="cpu")
    assert g.renderer is None


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


@pytest.mark.parametrize("flag_in_config", [True, False])
def test_combine_without_a_renderer_raises_up_front(flag_in_config):
    """No renderer with the flag set (by the config or the argument): the reference's ValueError, before any mask work -- the fake graph
    gives no rays, so reaching the aabb step would fail differently."""
    from signerf_amd import datasetgenerator as dg

    orig = dg._adopt
    dg._adopt = lambda c: c
    try:
        cfg = dg.DatasetGeneratorConfig(combine_shape_with_depth=flag_in_config)
        with pytest.raises(ValueError, match="Renderer is None but masking mode is shape"):
            dg.render_camera(cfg, _Graph(), _Cam(), combine_shape_with_depth=None if flag_in_config else True)
    finally:
        dg._adopt = orig


# ---- pinning against pyrender (tools/make_pyrender_fixture.py) -------------------------------------------------------------------------
def _fixture_names():
    return sorted(f for f in os.listdir(GOLDEN) if f.endswith(".npz")) if os.path.isdir(GOLDEN) else []


@pytest.mark.skipif(not _fixture_names(), reason="no pyrender fixtures yet: run tools/make_pyrender_fixture.py where pyrender and trimesh "
                                                 "are installed")
@pytest.mark.parametrize("name", _fixture_names() or ["none"])
def test_shading_constants_against_pyrender_fixture(name):
    """Where tools/make_pyrender_fixture.py has recorded what pyrender draws, the shading restatement (the UNPINNED constants of
    signerf_amd/renderer.py) must give the same colours away from silhouette edges (pyrender resolves a multisampled image there)."""
    z = np.load(os.path.join(GOLDEN, name))
    v, f, mv = z["vertices"], z["triangles"], z["model_view"]
    vc = z["vertex_colors"] if z["vertex_colors"].size else None
    fx, fy, cx, cy = (float(a) for a in z["intrinsics"])
    H, W = z["color"].shape[:2]
    tri, depth, bary, gap = mco.raster_front(v, f, mv, fx, fy, cx, cy, H, W)
    _, amb, graze = mo.raster_depth(v, f, mv, fx, fy, cx, cy, H, W)
    interior = ~amb & ~graze & (gap > 1e-3)
    edge = np.zeros_like(interior)   # one pixel around every coverage change: MSAA blends the silhouette
    cov = tri >= 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            edge |= np.roll(np.roll(cov, dy, 0), dx, 1) != cov
    ok = interior & ~edge
    x = mco.shade(tri, bary, f, vc, **shade_defaults(vc is not None))
    got = z["color"].astype(np.int64)
    assert ok.sum() > 100
    assert (np.abs(got - np.floor(x + 0.5)) <= 1)[ok].all()
    assert ((z["depth"] > 0) == cov)[ok].all()
