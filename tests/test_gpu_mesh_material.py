"""Proxy-mesh materials on the GPU (``RendererConfig.materials = "mtl"``): ``sn_mesh_raster_color_materials`` and
``sn_mesh_cast_rays_materials`` against the float64 oracle (tests/mesh_material_oracle.py), against the kernels they extend (depth and
default-grey colour bit for bit) and against each other, and ``render_camera`` / ``generate_dataset`` end to end.

Scenes: the ``CASES`` meshes of tests/test_gpu_mesh_color.py for the raster and the bunny stand-in under four views of
tests/test_gpu_mesh_rays.py for the ray cast, so the geometry -- and every ambiguity flag -- is the one those files use; the caps on the
flagged shares are checked on the CPU by tests/test_mesh_material_host.py and again here.  OBJ, MTL and the procedural textures are
written to tmp_path and read back by the package's own readers.  Each test prints its figures before it asserts."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mesh_color_oracle as mco
import mesh_material_oracle as mmo
import mesh_oracle as mo
import mesh_rays_oracle as mro
from helpers import make_model, small_config
from signerf_amd import Cameras, scene
from signerf_amd.datasetgenerator import DatasetGeneratorConfig, aabb_mask_and_condition, render_camera
from signerf_amd.renderer import (PYRENDER_DEFAULT_BASE_COLOR, Renderer, RendererConfig, cast_rays, cast_rays_materials, load_obj,
                                  load_obj_materials, model_view, object_pose, pack_materials, raster_color, raster_color_materials, raster_depth)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = mro.views()


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _caps(name, ok, covered):
    of_pixels, of_covered = mro.flagged_shares(~ok, covered)
    print(f"{name}: covered {covered.mean():.4f}; flagged {int((~ok).sum())} = {of_pixels:.5f} of the pixels (cap {mro.MAX_FLAGGED_OF_PIXELS}), "
          f"{of_covered:.5f} of the covered (cap {mro.MAX_FLAGGED_OF_COVERED})")
    assert of_pixels <= mro.MAX_FLAGGED_OF_PIXELS and of_covered <= mro.MAX_FLAGGED_OF_COVERED


def _load(path, gpu):
    """What the package reads from the scene files -> (v, f, tensors, MeshMaterials, corner_uv, triangle_material)."""
    v, f = load_obj(path)
    uv, tm, mats = load_obj_materials(path)
    return v, f, torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), pack_materials(uv, tm, mats), uv, tm


def _textured_scene(tmp_path, name, v, f):
    files, mats = mmo.textured_materials()
    uv, tm = mmo.spherical_corner_uv(v, f), mmo.thirds(f.shape[0])
    return mmo.write_scene(str(tmp_path), name, v, f, uv, tm, files), uv, tm, mats


def _camera(view, gpu):
    d = None if view["distortion"] is None else torch.tensor(view["distortion"], dtype=torch.float32)
    return Cameras(torch.from_numpy(view["c2w"])[None], view["fx"], view["fy"], view["cx"], view["cy"], view["W"], view["H"], distortion_params=d,
                   camera_type=view["camera_type"]).to(gpu)[0]


@pytest.fixture(scope="module")
def bunny(gpu, tmp_path_factory):
    """The bunny stand-in with the three textured-scene materials, as one OBJ + MTL + two PNG -> (v, f, world, uv, tm, oracle materials,
    renderers by (lens, materials))."""
    v, f, _ = mro.bumpy_sphere()
    d = tmp_path_factory.mktemp("bunny_mtl")
    obj, uv, tm, mats = _textured_scene(d, "bunny", v, f)
    rs = {}
    for lens in ("pinhole", "camera"):
        for m in ("none", "mtl"):
            rs[lens, m] = Renderer(RendererConfig(scale=mro.BUNNY_SCALE, object_path=obj, lens=lens, materials=m), device=gpu)
            rs[lens, m].setup()
    np.testing.assert_array_equal(rs["pinhole", "mtl"]._host_mesh[0], v)
    np.testing.assert_array_equal(rs["pinhole", "mtl"]._host_materials.corner_uv, uv)
    return v, f, mro.posed(v, object_pose(rs["pinhole", "mtl"].config)), uv, tm, mats, rs


# ---- (G1) identity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("name", sorted(mmo.RASTER_CASES))
def test_g1_one_default_grey_material_is_the_plain_colour_raster(gpu, tmp_path, name, cull):
    mesh, mv, fx, fy, cx, cy, H, W = mmo.RASTER_CASES[name]
    v, f = mesh()
    path = mmo.write_scene(str(tmp_path), name, v, f, None, np.zeros(f.shape[0], np.int32), [("grey", PYRENDER_DEFAULT_BASE_COLOR[:3], None, None)])
    v2, f2, tv, tf, mm, _, _ = _load(path, gpu)
    np.testing.assert_array_equal(v2, v)
    want_c, _ = raster_color(tv, tf, mv, fx, fy, cx, cy, H, W, cull_back_faces=cull)
    want_d = raster_depth(tv, tf, mv, fx, fy, cx, cy, H, W, cull_back_faces=cull)
    color, depth = raster_color_materials(tv, tf, mv, fx, fy, cx, cy, H, W, mm, cull_back_faces=cull)
    assert color.shape == (H, W, 3) and color.dtype == torch.uint8 and torch.equal(color, want_c) and _bits(depth, want_d)
    assert int((want_d > 0).sum()) > 500 and (color[(want_d > 0)[..., 0]] == 148).all()
    c2, none = raster_color_materials(tv, tf, mv, fx, fy, cx, cy, H, W, mm, cull_back_faces=cull, with_depth=False)
    assert none is None and torch.equal(c2, color)


@pytest.mark.parametrize("cull", [True, False])
def test_g1_one_default_grey_material_is_the_plain_ray_cast(gpu, bunny, cull):
    v, f, world, uv, tm, mats, rs = bunny
    r = rs["camera", "none"]
    grey = pack_materials(None, np.zeros(f.shape[0], np.int32), [__import__("signerf_amd.renderer", fromlist=["x"]).ObjMaterial("grey", (0.3, 0.3, 0.3))])
    cam = _camera(VIEWS["fisheye_4_512"], gpu)
    b = cam.generate_rays(camera_indices=0)
    fwd = mro.forward_of(VIEWS["fisheye_4_512"]["c2w"])
    _, tris = r.mesh_on(gpu)
    want_c, want_d = cast_rays(b.origins, b.directions, fwd, r.accel_on(gpu), f.shape[0], 512, 512, tris, None, 0, True, cull_back_faces=cull)
    color, depth = cast_rays_materials(b.origins, b.directions, fwd, r.accel_on(gpu), f.shape[0], 512, 512, grey, cull_back_faces=cull)
    assert torch.equal(color, want_c) and _bits(depth, want_d) and int((want_d > 0).sum()) > 500


# ---- (G2) Kd only ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mmo.RASTER_CASES))
def test_g2_kd_only_is_exact(gpu, tmp_path, name):
    mesh, mv, fx, fy, cx, cy, H, W = mmo.RASTER_CASES[name]
    v, f = mesh()
    x = 255.0 * np.power(np.asarray(mmo.KD_EXACT, dtype=np.float64), 1.0 / 2.2)
    assert (np.abs(x - np.floor(x) - 0.5) > 1e-3).all()   # fp32 powf cannot land on the other side of a rounding boundary
    want_m = np.floor(x + 0.5).astype(np.int64)            # [3 materials, 3 channels]
    tm = mmo.thirds(f.shape[0])
    path = mmo.write_scene(str(tmp_path), name, v, f, None, tm, [(f"m{k}", kd, None, None) for k, kd in enumerate(mmo.KD_EXACT)])
    _, _, tv, tf, mm, uv, tm2 = _load(path, gpu)
    assert uv is None and (tm2 == tm).all()
    color, depth = raster_color_materials(tv, tf, mv, fx, fy, cx, cy, H, W, mm)
    got, cov = color.cpu().numpy().astype(np.int64), depth[..., 0].cpu().numpy() > 0
    tri, bary, ok, ocov = mmo.raster_flags(v, f, mv, fx, fy, cx, cy, H, W)
    _caps(name, ok, ocov)
    assert not ((cov != ocov) & ok).any()
    sel = ok & ocov
    assert sel.sum() > 500 and (got[sel] == want_m[tm[tri[sel]]]).all() and (got[~cov] == 255).all()
    assert len(np.unique(got[sel], axis=0)) == 3 and not (got[sel] == 148).all()


# ---- (G3) textured: against the oracle -----------------------------------------------------------------------------------------------------------
def _check_textured(name, got, cov, x, spread, ok, ocov):
    _caps(name, ok, ocov)
    assert not ((cov != ocov) & ok).any(), f"{int(((cov != ocov) & ok).sum())} pixels differ in coverage off the flags"
    sel = ok & ocov
    bad, worst = mmo.compare(got, x, spread, sel, mmo.MAX_SIDE)
    n_col = len(np.unique(got[sel], axis=0))
    one = int(((np.abs(got - np.floor(x + 0.5)) == 1).any(-1) & sel).sum())
    print(f"{name}: {int(sel.sum())} pixels compared, {n_col} distinct colours, largest difference {worst} level(s), {one} pixels one level off "
          f"(all of them ties: {not bad.any()}), largest spread {spread[sel].max():.1f} levels, largest tie window {mmo.tie_window(spread[sel].max(), mmo.MAX_SIDE):.4f}")
    assert not bad.any(), f"{int(bad.any(-1).sum())} pixels differ, e.g. {np.argwhere(bad)[:4].tolist()}"
    assert sel.sum() > 500 and n_col > 20   # non-vacuous
    assert (got[~cov & ok] == 255).all()


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("name", sorted(mmo.RASTER_CASES))
def test_g3_textured_raster_against_the_oracle(gpu, tmp_path, name, cull):
    mesh, mv, fx, fy, cx, cy, H, W = mmo.RASTER_CASES[name]
    v, f = mesh()
    path, uv, tm, mats = _textured_scene(tmp_path, name, v, f)
    _, _, tv, tf, mm, uv2, tm2 = _load(path, gpu)
    np.testing.assert_array_equal(uv2, uv)
    assert (tm2 == tm).all() and mm.textured and mm.records["tex_width"].tolist() == [64, 96, 0]
    color, depth = raster_color_materials(tv, tf, mv, fx, fy, cx, cy, H, W, mm, cull_back_faces=cull)
    assert _bits(depth, raster_depth(tv, tf, mv, fx, fy, cx, cy, H, W, cull_back_faces=cull))
    tri, bary, ok, ocov = mmo.raster_flags(v, f, mv, fx, fy, cx, cy, H, W, cull=cull)
    x, spread = mmo.shade(tri, bary, uv, tm, mats)
    _check_textured(f"{name} cull={cull}", color.cpu().numpy().astype(np.int64), depth[..., 0].cpu().numpy() > 0, x, spread, ok, ocov)


@pytest.mark.parametrize("name", mmo.RAY_VIEWS)
def test_g3_textured_ray_cast_against_the_oracle(gpu, bunny, name):
    v, f, world, uv, tm, mats, rs = bunny
    view = VIEWS[name]
    cam = _camera(view, gpu)
    H, W = view["H"], view["W"]
    color, depth = rs["camera", "mtl"].render_camera(cam, with_color=True)
    assert color.shape == (H, W, 3) and color.dtype == torch.uint8
    b = cam.generate_rays(camera_indices=0)
    o, d = b.origins.cpu().numpy().reshape(-1, 3), b.directions.cpu().numpy().reshape(-1, 3)
    tri, bary, ok, z = mmo.ray_flags(o, d, mro.forward_of(view["c2w"]), world, f)
    x, spread = mmo.shade(tri.reshape(H, W), bary.reshape(H, W, 3), uv, tm, mats)
    _check_textured(name, color.cpu().numpy().astype(np.int64), depth[..., 0].cpu().numpy() > 0, x, spread, ok.reshape(H, W), (z > 0).reshape(H, W))


# ---- (G4) the two paths agree on a pinhole ---------------------------------------------------------------------------------------------------------
def test_g4_pinhole_raster_and_ray_cast_agree(gpu, bunny):
    v, f, world, uv, tm, mats, rs = bunny
    name = "pinhole_1_531x397"
    view = VIEWS[name]
    cam = _camera(view, gpu)
    H, W = view["H"], view["W"]
    c_ray, d_ray = rs["camera", "mtl"].render_camera(cam, with_color=True)
    c_ras, d_ras = rs["pinhole", "mtl"].render_camera(cam, with_color=True)
    b = cam.generate_rays(camera_indices=0)
    z, tri, edge, _ = mro.cast(b.origins.cpu().numpy(), b.directions.cpu().numpy(), mro.forward_of(view["c2w"]), world, f)
    mv = model_view(view["c2w"].reshape(-1).tolist(), object_pose(rs["pinhole", "mtl"].config))
    _, amb, graze = mo.raster_depth(v, f, mv, view["fx"], view["fy"], view["cx"], view["cy"], H, W)
    ok = (~(edge < mro.EPS)).reshape(H, W) & ~amb & ~graze
    _caps(name, ok, (z > 0).reshape(H, W))
    dc = np.abs(c_ray.cpu().numpy().astype(int) - c_ras.cpu().numpy().astype(int))
    print(f"{name}: raster and ray cast differ by at most {dc[ok].max()} of 255 off the flags ({int((dc.max(-1) > 0)[ok].sum())} pixels differ at all)")
    assert dc[ok].max() <= 1 and int(ok.sum()) > 500
    assert len(np.unique(c_ray.cpu().numpy()[ok & (z > 0).reshape(H, W)], axis=0)) > 20


# ---- (G5) determinism, and the depth does not change -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens,name", [("pinhole", "pinhole_1_531x397"), ("pinhole", "opencv_2_640x480"), ("camera", "opencv_2_640x480"),
                                       ("camera", "equirect_512x256")])
def test_g5_deterministic_and_depth_is_the_none_depth(gpu, bunny, lens, name):
    v, f, world, uv, tm, mats, rs = bunny
    cam = _camera(VIEWS[name], gpu)
    c1, d1 = rs[lens, "mtl"].render_camera(cam, with_color=True)
    c2, d2 = rs[lens, "mtl"].render_camera(cam, with_color=True)
    assert torch.equal(c1, c2) and _bits(d1, d2)
    c0, d0 = rs[lens, "none"].render_camera(cam, with_color=True)
    assert _bits(d1, d0) and _bits(rs[lens, "mtl"].render_camera(cam)[1], d0) and _bits(rs[lens, "none"].render_camera(cam)[1], d0)
    cov = (d0 > 0)[..., 0]
    assert int(cov.sum()) > 500 and (c0[cov] == 148).all() and not (c1[cov] == 148).all() and torch.equal(c1[~cov], c0[~cov])


# ---- (G6) end to end -----------------------------------------------------------------------------------------------------------------------------
def test_g6_render_camera_combine_end_to_end(gpu, tmp_path):
    v, f = mo.icosphere(3)
    obj, uv, tm, mats = _textured_scene(tmp_path, "ico", v, f)
    model, _ = make_model(small_config(num_proposal_iterations=0, num_nerf_samples_per_ray=32), gpu, density_bias=5.0)
    H = W = 96
    cams = Cameras(scene.benchmark_cameras(8)[:, :3], 130.0, 130.0, W / 2, H / 2, W, H).to(gpu)
    box = dict(aabb_min=[-0.25, -0.25, -0.25], aabb_max=[0.25, 0.25, 0.25], mask_dialation=(11, 11))
    place = dict(position=[0.0, 0.0, 0.05], scale=[0.02, 0.02, 0.02], object_path=obj)
    n_diff = 0
    for lens in ("pinhole", "camera"):
        rm = Renderer(RendererConfig(materials="mtl", lens=lens, **place), device=gpu)
        rn = Renderer(RendererConfig(lens=lens, **place), device=gpu)
        rm.setup()
        rn.setup()
        gen_m = DatasetGeneratorConfig(combine_shape_with_depth=True, renderer=rm.config, **box)
        gen_n = DatasetGeneratorConfig(combine_shape_with_depth=True, renderer=rn.config, **box)
        for k in (0, 3):
            rgb, mask, cond = render_camera(gen_m, model, cams[k], renderer=rm)
            rgb_n, mask_n, cond_n = render_camera(gen_n, model, cams[k], renderer=rn)
            bundle = cams[k].generate_rays(0, aabb_box=model.render_aabb)
            depth = model.eval().get_outputs_for_camera_ray_bundle(bundle)["depth"]
            model.train()
            aabb = torch.tensor([gen_m.aabb_min, gen_m.aabb_max])
            pmask, _ = aabb_mask_and_condition(depth, bundle.origins, bundle.directions, aabb, gen_m.mask_dialation)
            assert torch.equal(mask, pmask) and torch.equal(mask, mask_n) and torch.equal(rgb, rgb_n) and mask.any()   # the plain aabb mask
            color, md = rm.render_camera(cams[k], with_color=True)
            plain_bundle = cams[k].generate_rays(0)
            rmask, rcond = mco.combined_mask_and_condition(depth.cpu(), plain_bundle.origins.cpu(), plain_bundle.directions.cpu(), aabb, md.cpu(),
                                                           color.cpu(), gen_m.mask_dialation)
            assert torch.equal(mask.cpu(), rmask) and _bits(cond.cpu(), rcond)
            cv = (md < depth) & (md > 0)
            differs = ~((cond == cond_n) | (torch.isnan(cond) & torch.isnan(cond_n)))
            assert not (differs & ~cv).any()   # nowhere outside cv
            grey = 1 - torch.tensor([148], dtype=torch.uint8, device=gpu) / 255.0
            assert (cond_n[cv] == grey).all()   # "none" on the same OBJ + MTL: the parent commit's 148
            n_diff += int((differs & cv).sum())
    print(f"the materials change the condition on {n_diff} pixels inside cv")
    assert n_diff > 50


SIZE, N_VIEWS = 64, 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setup(dev, obj, materials):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import make_model, small_config
    from signerf_amd import random_sphere_poses, scene
    from signerf_amd.datasetgenerator import DatasetGenerator, DatasetGeneratorConfig
    from signerf_amd.renderer import RendererConfig

    cfg = small_config(num_proposal_samples_per_ray=(64, 32), num_nerf_samples_per_ray=24)
    model, _ = make_model(cfg, dev, density_bias=5.0)
    ref = scene.benchmark_cameras(8)[:, :3]
    torch.manual_seed(1)
    syn = random_sphere_poses(N_VIEWS, torch.device("cpu"), 0.5, (30.0, 120.0), (0.0, 360.0), [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])[:, :3]

    def generator(path, name, **kw):
        c = DatasetGeneratorConfig(path=path, dataset_name=name, fx=1.2 * SIZE, fy=1.2 * SIZE, cx=SIZE / 2, cy=SIZE / 2, width=SIZE,
                                   height=SIZE, rows=3, cols=3, mask_dialation=(7, 7), aabb_min=[-0.25, -0.25, -0.25],
                                   aabb_max=[0.25, 0.25, 0.25], combine_shape_with_depth=True,
                                   renderer=RendererConfig(position=[0.0, 0.0, 0.05], scale=[0.02, 0.02, 0.02], object_path=obj, materials=materials))
        return DatasetGenerator(c, torch.eye(4)[:3], 1.0, None, device=dev, **kw)

    return model, ref, syn, generator


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(d, fn)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    out.pop("config.yml", None)   # (holds the dataset name)
    return out


def _worker(rank, world, port, out_dir, obj):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model, ref, syn, generator = _setup(dev, obj, "mtl")
    generator(out_dir, "sharded").generate_dataset(model, ref, synthetic_camera_to_worlds=syn)
    dist.destroy_process_group()


def test_g6_generate_dataset_one_vs_two_processes_and_none_is_the_parent(gpu, tmp_path):
    v, f = mo.icosphere(2)
    obj, uv, tm, mats = _textured_scene(tmp_path, "ico", v, f)
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), obj), nprocs=2, join=True)
    model, ref, syn, generator = _setup(gpu, obj, "mtl")
    g = generator(tmp_path, "single")
    g.generate_dataset(model, ref, synthetic_camera_to_worlds=syn)
    assert g.renderer._host_materials is not None and g.renderer._host_materials.textured
    a, b = _tree(tmp_path / "sharded"), _tree(tmp_path / "single")
    assert a.keys() == b.keys() and len(a) == 1 + 4 + 8 * (8 + N_VIEWS)
    for k in a:
        assert a[k] == b[k], f"{k}: two-process dataset differs from the single-process one"
    import yaml

    assert yaml.safe_load((tmp_path / "single" / "config.yml").read_text())["renderer"]["materials"] == "mtl"
    # "none" on the same OBJ + MTL writes what the parent commit writes: the bytes of the same mesh without any material line
    _, _, _, gen_none = _setup(gpu, obj, "none")
    gen_none(tmp_path, "none").generate_dataset(model, ref, synthetic_camera_to_worlds=syn)
    bare = str(tmp_path / "bare.obj")
    with open(bare, "w") as fh:
        fh.write("".join(f"v {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in v.tolist()) + "".join(f"f {p + 1} {q + 1} {r + 1}\n" for p, q, r in f.tolist()))
    _, _, _, gen_bare = _setup(gpu, bare, "none")
    gen_bare(tmp_path, "bare").generate_dataset(model, ref, synthetic_camera_to_worlds=syn)
    n, p = _tree(tmp_path / "none"), _tree(tmp_path / "bare")
    assert n.keys() == p.keys() == b.keys() and all(n[k] == p[k] for k in n)
    assert any(n[k] != b[k] for k in b if k.startswith("conditions")) and all(n[k] == b[k] for k in b if k.startswith("masks"))
