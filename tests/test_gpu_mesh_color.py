"""combine_shape_with_depth on the GPU: ``sn_mesh_raster_color`` against the float64 restatement of the shading (tests/mesh_color_oracle.py)
and against ``sn_mesh_raster_depth`` (its depth bit for bit), ``sn_aabb_mask_condition_combined`` against the restatement of
datasetgenerator.py:794-811 (bit-exact), and ``render_camera`` / ``generate_dataset`` with the flag end to end."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mesh_color_oracle as mco
import mesh_oracle as mo
from helpers import make_model, small_config
from oracle import nerfacto as onf
from oracle import signerf_utils as su
from signerf_amd import Cameras, scene
from signerf_amd.datasetgenerator import (DatasetGeneratorConfig, aabb_mask_and_condition, aabb_mask_and_condition_combined,
                                          render_camera)
from signerf_amd.renderer import Renderer, RendererConfig, model_view, object_pose, raster_color, raster_depth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mv(t=(0.0, 0.0, 0.0)):
    return np.hstack([np.eye(3), np.asarray(t, dtype=np.float64).reshape(3, 1)])


def _same_bits(a, b):
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


CASES = {
    # name: (mesh, mv, fx, fy, cx, cy, H, W)
    "icosphere": (lambda: mo.icosphere(3), _mv((0.1, -0.05, -3.0)), 100.0, 100.0, 64.0, 48.0, 96, 128),
    "soup": (lambda: mo.triangle_soup(300, seed=1), _mv(), 80.0, 80.0, 64.0, 48.0, 96, 128),
    "close_up": (lambda: mo.triangle_soup(400, seed=2, center=(0.0, 0.0, -5.0), spread=7.0, size=1.5), _mv(), 60.0, 60.0, 48.0, 48.0, 96, 96),
}


def _up(gpu, v, f, vc=None):
    return torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), None if vc is None else torch.from_numpy(vc).to(gpu)


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_color_raster_depth_is_bit_identical(gpu, name, cull):
    mesh, mv, fx, fy, cx, cy, H, W = CASES[name]
    v, f = mesh()
    tv, tf, tc = _up(gpu, v, f, mco.position_colors(v))
    want = raster_depth(tv, tf, mv, fx, fy, cx, cy, H, W, cull_back_faces=cull)
    for vc in (None, tc):
        color, depth = raster_color(tv, tf, mv, fx, fy, cx, cy, H, W, vc, cull_back_faces=cull)
        assert color.shape == (H, W, 3) and color.dtype == torch.uint8 and depth.shape == (H, W, 1)
        assert torch.equal(depth.view(torch.int32), want.view(torch.int32))
    assert int((want > 0).sum()) > 500


def test_color_raster_depth_is_bit_identical_800(gpu):
    """The one full-size frame: a bunny-sized (~70k triangles) closed mesh at 800 x 800."""
    v, f = mo.icosphere(6, 0.8)
    tv, tf, _ = _up(gpu, v, f)
    mv = _mv((0.05, -0.02, -2.2))
    want = raster_depth(tv, tf, mv, 800.0, 800.0, 400.0, 400.0, 800, 800)
    color, depth = raster_color(tv, tf, mv, 800.0, 800.0, 400.0, 400.0, 800, 800)
    assert torch.equal(depth.view(torch.int32), want.view(torch.int32))
    cov = (want[..., 0] > 0).cpu()
    c = color.cpu()
    assert int(cov.sum()) > 100_000 and (c[cov] == 148).all() and (c[~cov] == 255).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_color_without_vertex_colors_is_the_constant(gpu, name):
    """No vertex colours: pyrender's default grey (0.3) under ambient 1 with gamma -> 148 on every covered pixel, white elsewhere;
    coverage against the float64 oracle away from ambiguous pixels, as the depth test gates it."""
    mesh, mv, fx, fy, cx, cy, H, W = CASES[name]
    v, f = mesh()
    tv, tf, _ = _up(gpu, v, f)
    color, depth = raster_color(tv, tf, mv, fx, fy, cx, cy, H, W)
    c, d = color.cpu().numpy(), depth[..., 0].cpu().numpy()
    cov = d > 0
    assert (c[cov] == 148).all() and (c[~cov] == 255).all()
    ref, amb, _ = mo.raster_depth(v, f, mv, fx, fy, cx, cy, H, W, cull=True)
    assert not ((cov != (ref > 0)) & ~amb).any()
    # other shading parameters reach the kernel: no gamma, a coloured ambient light, a black background
    c2, _ = raster_color(tv, tf, mv, fx, fy, cx, cy, H, W, base_color=(0.6, 0.25, 1.0, 1.0), ambient=(1.0, 0.5, 0.2), background=(0, 0, 0),
                         gamma=False, with_depth=False)
    c2 = c2.cpu().numpy()
    want = np.array([153, 32, 51])   # round(255 * (0.6, 0.125, 0.2))
    assert (c2[cov] == want).all() and (c2[~cov] == 0).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_color_with_vertex_colors_matches_oracle(gpu, name):
    mesh, mv, fx, fy, cx, cy, H, W = CASES[name]
    v, f = mesh()
    vc = mco.position_colors(v)
    tv, tf, tc = _up(gpu, v, f, vc)
    color, depth = raster_color(tv, tf, mv, fx, fy, cx, cy, H, W, tc, base_color=(1.0, 1.0, 1.0, 1.0))
    got = color.cpu().numpy().astype(np.int64)
    tri, od, bary, gap = mco.raster_front(v, f, mv, fx, fy, cx, cy, H, W)
    x = mco.shade(tri, bary, f, vc, base_color=(1.0, 1.0, 1.0, 1.0))
    _, amb, graze = mo.raster_depth(v, f, mv, fx, fy, cx, cy, H, W, cull=True)
    ok = ~amb & ~graze & (gap > 1e-4)   # the front triangle is well defined
    cov = depth[..., 0].cpu().numpy() > 0
    assert not ((cov != (tri >= 0)) & ~amb).any()
    want = np.floor(x + 0.5).astype(np.int64)
    tie = np.abs(x - np.floor(x) - 0.5) < 1e-3
    diff = np.abs(got - want)
    bad = ok[..., None] & ((diff > 1) | ((diff == 1) & ~tie))
    assert not bad.any(), f"{bad.any(-1).sum()} pixels differ, e.g. {np.argwhere(bad)[:4].tolist()}"
    assert int((ok & (tri >= 0)).sum()) > 500 and len(np.unique(got[cov].reshape(-1, 3), axis=0)) > 20   # non-vacuous


def test_coincident_triangles_lowest_index_wins(gpu):
    """Two triangles at the same place and depth, red and green: GL_LESS keeps the first drawn, i.e. the lower index."""
    tri = np.array([[-0.5, -0.5, -2.0], [0.5, -0.5, -2.0], [0.0, 0.5, -2.0]], np.float32)
    v = np.vstack([tri, tri])
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    vc = np.array([[255, 0, 0, 255]] * 3 + [[0, 255, 0, 255]] * 3, np.uint8)
    for order, want in ((f, [255, 0, 0]), (f[::-1].copy(), [0, 255, 0])):
        tv, tf, tc = _up(gpu, v, order, vc)
        color, depth = raster_color(tv, tf, _mv(), 40.0, 40.0, 16.0, 16.0, 32, 32, tc, base_color=(1.0, 1.0, 1.0, 1.0))
        cov = (depth[..., 0] > 0).cpu()
        assert int(cov.sum()) > 50 and (color.cpu()[cov] == torch.tensor(want, dtype=torch.uint8)).all()


def _write_obj(path, v, f, vc=None):
    with open(path, "w") as fh:
        if vc is None:
            fh.write("".join(f"v {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in v.tolist()))
        else:
            fh.write("".join(f"v {x:.9g} {y:.9g} {z:.9g} {r / 255:.9g} {g / 255:.9g} {b / 255:.9g}\n"
                             for (x, y, z), (r, g, b, _) in zip(v.tolist(), vc.tolist())))
        fh.write("".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f.tolist()))


@pytest.mark.parametrize("colored", [False, True])
def test_renderer_color_deterministic_and_no_sync(gpu, tmp_path, colored):
    v, f = mo.icosphere(3)
    vc = mco.position_colors(v) if colored else None
    _write_obj(tmp_path / "ico.obj", v, f, vc)
    cfg = RendererConfig(position=[0.02, -0.03, 0.01], rotation=[20, 40, -30], scale=[0.012, 0.008, 0.01], object_path=str(tmp_path / "ico.obj"))
    r = Renderer(cfg, device=gpu)
    r.setup()
    H, W = 72, 96
    cams = Cameras(scene.benchmark_cameras(8)[:, :3], 90.0, 90.0, W / 2, H / 2, W, H).to(gpu)
    first = r.render_camera(cams[1], with_color=True)   # the first colour view on this device uploads the mesh and its colours
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = r.render_camera(cams[1], with_color=True)
        other = r.render_camera(cams[5], with_color=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))
    _, d_only = r.render_camera(cams[5])
    assert torch.equal(other[1].view(torch.int32), d_only.view(torch.int32))
    color = other[0].cpu().numpy()
    cov = d_only[..., 0].cpu().numpy() > 0
    assert cov.sum() > 100 and (color[~cov] == 255).all()
    if not colored:
        assert (color[cov] == 148).all()
    else:   # base colour 1 with vertex colours: the oracle given the same matrices
        mv = model_view(cams._host[5, :12].tolist(), object_pose(cfg))
        tri, _, bary, gap = mco.raster_front(v, f, mv, 90.0, 90.0, W / 2, H / 2, H, W)
        x = mco.shade(tri, bary, f, np.asarray(r._host_colors[0]), base_color=(1.0, 1.0, 1.0, 1.0))
        _, amb, graze = mo.raster_depth(v, f, mv, 90.0, 90.0, W / 2, H / 2, H, W)
        ok = (~amb & ~graze & (gap > 1e-4) & cov)[..., None] & (np.abs(x - np.floor(x) - 0.5) >= 1e-3)
        assert ok.sum() > 100 and (color.astype(np.int64) == np.floor(x + 0.5))[ok].all()


# ---- the combined aabb condition ------------------------------------------------------------------------------------------------------
def _scene(H, W, cam=1, focal=None, poison=False):
    c2w = scene.benchmark_cameras(8)
    r = onf.generate_rays(c2w[cam, :3], focal or 1.4 * W, focal or 1.4 * W, W / 2, H / 2, H, W)
    g = torch.Generator().manual_seed(H * W + cam)
    depth = 2.0 + torch.rand(H, W, 1, generator=g)
    y0, y1, x0, x1 = (3 * H) // 8, (5 * H) // 8, (3 * W) // 8, (5 * W) // 8
    depth[y0:y1, x0:x1] = 0.45 + 0.1 * torch.rand(y1 - y0, x1 - x0, 1, generator=g)
    depth[H // 2, 1] = 0.5
    # the mesh: a disc that overlaps the box patch and the background, in front of the NeRF in places and behind it in others
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    disc = ((yy - 0.45 * H) ** 2 + (xx - 0.55 * W) ** 2) < (min(H, W) / 3.5) ** 2
    md = torch.zeros(H, W, 1)
    md[..., 0][disc] = 0.3 + 0.4 * torch.rand(int(disc.sum()), generator=g)
    color = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    if poison:
        depth[H // 2, W // 2] = float("nan")
        depth[H // 2 + 1, W // 2] = float("inf")
        depth[2, W - 3] = float("nan")
        depth[3, W - 3] = -float("inf")
    return r["origins"], r["directions"], depth, md, color


AABB = torch.tensor([[-0.1, -0.1, -0.1], [0.1, 0.1, 0.1]])


@pytest.mark.parametrize("H,W,dil,inverse,manual,poison", [
    (120, 160, (50, 50), False, None, False),       # the reference's defaults
    (97, 131, (9, 5), False, None, False),          # ragged size, non-square element
    (64, 64, None, False, None, False),             # no dilation
    (80, 100, (21, 21), True, None, False),         # inverse mask
    (80, 100, (21, 21), False, (0.1, 0.9), False),  # manual depth range
    (64, 80, (7, 7), False, None, True),            # NaN / inf NeRF depths
    (64, 80, None, True, (0.2, 3.0), True),         # NaN / inf, inverse, manual
])
def test_combined_mask_and_condition_bit_exact(gpu, H, W, dil, inverse, manual, poison):
    o, d, depth, md, color = _scene(H, W, poison=poison)
    mask, cond = aabb_mask_and_condition_combined(depth.to(gpu), o.to(gpu), d.to(gpu), AABB, md.to(gpu), color.to(gpu), dil, inverse, manual, 0.1)
    rmask, rcond = mco.combined_mask_and_condition(depth, o, d, AABB, md, color, dil, inverse, manual, 0.1)
    pmask, pcond = aabb_mask_and_condition(depth.to(gpu), o.to(gpu), d.to(gpu), AABB, dil, inverse, manual, 0.1)
    assert mask.dtype == torch.bool and mask.shape == (H, W, 1) and cond.shape == (H, W, 1)
    assert torch.equal(mask, pmask) and torch.equal(mask.cpu(), rmask)   # the plain aabb mask, bit for bit
    assert _same_bits(cond, rcond)
    cv = ((md < depth) & (md > 0)).to(gpu)
    assert int(cv.sum()) > 20 and int((~cv & (md > 0).to(gpu)).sum()) > 20   # the mesh is in front in places and behind in others
    assert _same_bits(cond[~cv], pcond[~cv])   # off the mesh-in-front pixels: the plain condition
    if poison and not inverse:
        assert torch.isnan(cond[H // 2, W // 2]).all()
    m2, c2 = aabb_mask_and_condition_combined(depth.to(gpu), o.to(gpu), d.to(gpu), AABB, md.to(gpu), color.to(gpu), dil, inverse, manual, 0.1,
                                              with_condition=False)
    assert torch.equal(m2, mask) and c2 is None


def test_combined_mesh_behind_is_plain_and_empty_box_is_zero(gpu):
    o, d, depth, md, color = _scene(96, 96)
    behind = torch.where(md > 0, depth + 1.0, md)
    mask, cond = aabb_mask_and_condition_combined(depth.to(gpu), o.to(gpu), d.to(gpu), AABB, behind.to(gpu), color.to(gpu), (11, 11))
    pmask, pcond = aabb_mask_and_condition(depth.to(gpu), o.to(gpu), d.to(gpu), AABB, (11, 11))
    assert torch.equal(mask, pmask) and _same_bits(cond, pcond) and mask.any()
    far = torch.tensor([[5.0, 5.0, 5.0], [5.1, 5.1, 5.1]])
    mask, cond = aabb_mask_and_condition_combined(depth.to(gpu), o.to(gpu), d.to(gpu), far, md.to(gpu), color.to(gpu), (11, 11))
    assert not mask.any() and torch.equal(cond.cpu(), torch.zeros(96, 96, 1))


def test_render_camera_combine_end_to_end(gpu, tmp_path):
    """With the flag the condition differs from the plain aabb one exactly where the mesh is in front of the NeRF, and holds
    1 - colour[0] / 255 there (the default grey: 1 - 148 / 255)."""
    v, f = mo.icosphere(3)
    _write_obj(tmp_path / "ico.obj", v, f)
    cfg = small_config(num_proposal_iterations=0, num_nerf_samples_per_ray=32)
    model, _ = make_model(cfg, gpu, density_bias=5.0)
    H = W = 96
    cams = Cameras(scene.benchmark_cameras(8)[:, :3], 130.0, 130.0, W / 2, H / 2, W, H).to(gpu)
    rcfg = RendererConfig(position=[0.0, 0.0, 0.05], scale=[0.02, 0.02, 0.02], object_path=str(tmp_path / "ico.obj"))
    box = dict(aabb_min=[-0.25, -0.25, -0.25], aabb_max=[0.25, 0.25, 0.25], mask_dialation=(11, 11))
    gen = DatasetGeneratorConfig(combine_shape_with_depth=True, renderer=rcfg, **box)
    plain = DatasetGeneratorConfig(**box)
    r = Renderer(rcfg, device=gpu)
    r.setup()
    n_cv = 0
    for k in (0, 3):
        rgb, mask, cond = render_camera(gen, model, cams[k], renderer=r)
        rgb_p, mask_p, cond_p = render_camera(plain, model, cams[k])
        assert torch.equal(rgb, rgb_p) and torch.equal(mask, mask_p) and mask.any()
        color, md = r.render_camera(cams[k], with_color=True)
        depth = model.eval().get_outputs_for_camera_ray_bundle(cams[k].generate_rays(0, aabb_box=model.render_aabb))["depth"]
        model.train()
        cv = (md < depth) & (md > 0)
        differs = ~((cond == cond_p) | (torch.isnan(cond) & torch.isnan(cond_p)))
        assert torch.equal(differs & ~cv, torch.zeros_like(cv))   # nothing changes off the mesh-in-front pixels
        grey = 1 - torch.tensor([148], dtype=torch.uint8, device=gpu) / 255.0   # fp32, as the reference forms it
        assert (cond[cv] == grey).all() and (color[cv[..., 0]] == 148).all()
        n_cv += int((cv & differs).sum())
        bundle = cams[k].generate_rays(0)
        rmask, rcond = mco.combined_mask_and_condition(depth.cpu(), bundle.origins.cpu(), bundle.directions.cpu(),
                                                       torch.tensor([gen.aabb_min, gen.aabb_max]), md.cpu(), color.cpu(), gen.mask_dialation)
        assert torch.equal(mask.cpu(), rmask) and _same_bits(cond, rcond)
    assert n_cv > 50   # the sphere is in front of the NeRF somewhere, and the flag changes the condition there
    # the flag argument overrides the config's either way; no renderer raises the reference's error
    _, _, c_off = render_camera(gen, model, cams[0], renderer=r, combine_shape_with_depth=False)
    _, _, c_p = render_camera(plain, model, cams[0])
    assert _same_bits(c_off, c_p)
    _, _, c_on = render_camera(plain, model, cams[0], renderer=r, combine_shape_with_depth=True)
    _, _, c_g = render_camera(gen, model, cams[0], renderer=r)
    assert _same_bits(c_on, c_g)
    with pytest.raises(ValueError, match="Renderer is None"):
        render_camera(gen, model, cams[0])


# ---- generate_dataset, one process vs two ---------------------------------------------------------------------------------------------
SIZE, N_VIEWS = 64, 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setup(dev, obj):
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
                                   renderer=RendererConfig(position=[0.0, 0.0, 0.05], scale=[0.02, 0.02, 0.02], object_path=obj))
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
    model, ref, syn, generator = _setup(dev, obj)
    generator(out_dir, "sharded").generate_dataset(model, ref, synthetic_camera_to_worlds=syn)
    dist.destroy_process_group()


def test_generate_dataset_combine_one_vs_two_processes(gpu, tmp_path):
    v, f = mo.icosphere(2)
    obj = str(tmp_path / "ico.obj")
    _write_obj(obj, v, f)
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), obj), nprocs=2, join=True)
    model, ref, syn, generator = _setup(gpu, obj)
    g = generator(tmp_path, "single")
    assert g.renderer is not None
    g.generate_dataset(model, ref, synthetic_camera_to_worlds=syn)
    a, b = _tree(tmp_path / "sharded"), _tree(tmp_path / "single")
    assert a.keys() == b.keys() and len(a) == 1 + 4 + 8 * (8 + N_VIEWS)
    for k in a:
        assert a[k] == b[k], f"{k}: two-process dataset differs from the single-process one"
    import yaml

    y = yaml.safe_load((tmp_path / "single" / "config.yml").read_text())
    assert y["masking_mode"] == "aabb" and y["combine_shape_with_depth"] is True and y["renderer"]["object_path"] == obj
    # the flag reached the written conditions: a plain run differs from them, with the same masks
    plain = generator(tmp_path, "plain")
    plain.config.combine_shape_with_depth = plain.combine_shape_with_depth = False
    plain.renderer = None
    plain.generate_dataset(model, ref, synthetic_camera_to_worlds=syn)
    p = _tree(tmp_path / "plain")
    assert p.keys() == b.keys()
    assert any(p[k] != b[k] for k in b if k.startswith("conditions")) and all(p[k] == b[k] for k in b if k.startswith("masks"))
