"""Lens-aware proxy mesh on the GPU: ``sn_mesh_cast_rays`` (``RendererConfig.lens = "camera"``) against the rasteriser for a pinhole,
against the brute-force float64 oracle (tests/mesh_rays_oracle.py) for every lens, and end to end through ``render_camera`` /
``generate_dataset``.

The mesh is the bunny's stand-in (``mesh_rays_oracle.bumpy_sphere``: 5 120 faces, radius about 0.15, with vertex colours), the views
are ``mesh_rays_oracle.views()``.  EPS (which rays are edge-flagged), Z_RTOL and the caps on the flagged shares are derived in the
docstring of tests/test_mesh_rays_host.py, on the CPU; each test prints its figures before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_oracle as mo
import mesh_rays_oracle as mro
from helpers import make_model, small_config
from signerf_amd import Cameras, _lib
from signerf_amd.datasetgenerator import (DatasetGenerator, DatasetGeneratorConfig, aabb_mask_and_condition_combined, render_camera,
                                          shape_mask_and_condition)
from signerf_amd.renderer import Renderer, RendererConfig, cast_rays, model_view, object_pose
from mesh_rays_oracle import EPS, Z_RTOL

pytestmark = pytest.mark.gpu

VIEWS = mro.views()
PINHOLE = [k for k in VIEWS if k.startswith("pinhole")]
LENSES = [k for k in VIEWS if not k.startswith("pinhole")]


def _write_obj(path, v, f, col):
    with open(path, "w") as fh:
        fh.write("".join(f"v {x:.9g} {y:.9g} {z:.9g} {r:.6f} {g:.6f} {b:.6f}\n" for (x, y, z), (r, g, b) in zip(v.tolist(), col.tolist())))
        fh.write("".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f.tolist()))


@pytest.fixture(scope="module")
def bunny(gpu, tmp_path_factory):
    """(mesh, posed vertices, the pinhole renderer, the lens-aware renderer) of one OBJ file."""
    v, f, col = mro.bumpy_sphere()
    obj = str(tmp_path_factory.mktemp("bunny") / "bunny.obj")
    _write_obj(obj, v, f, col)
    out = []
    for lens in ("pinhole", "camera"):
        r = Renderer(RendererConfig(scale=mro.BUNNY_SCALE, object_path=obj, lens=lens), device=gpu)
        r.setup()
        out.append(r)
    hv, hf = out[0]._host_mesh
    np.testing.assert_array_equal(hv, v)
    return (v, f), mro.posed(v, object_pose(out[0].config)), out[0], out[1]


def _camera(view, gpu):
    d = None if view["distortion"] is None else torch.tensor(view["distortion"], dtype=torch.float32)
    cams = Cameras(torch.from_numpy(view["c2w"])[None], view["fx"], view["fy"], view["cx"], view["cy"], view["W"], view["H"], distortion_params=d,
                   camera_type=view["camera_type"]).to(gpu)
    return cams[0]


def _oracle(cam, view, world, f):
    """The float64 oracle from the fp32 rays the GPU generated for `cam`."""
    b = cam.generate_rays(camera_indices=0)
    z, tri, edge, ff = mro.cast(b.origins.cpu().numpy(), b.directions.cpu().numpy(), mro.forward_of(view["c2w"]), world, f)
    return b, z, tri, edge, ff


def _check_caps(name, flag, covered):
    of_pixels, of_covered = mro.flagged_shares(flag, covered)
    print(f"{name}: covered {covered.mean():.4f} of the view; flagged {int(flag.sum())} = {of_pixels:.5f} of the pixels (cap "
          f"{mro.MAX_FLAGGED_OF_PIXELS}), {of_covered:.5f} of the covered (cap {mro.MAX_FLAGGED_OF_COVERED})")
    assert covered.mean() >= 0.05, "the mesh covers too little of the view for the test to mean anything"
    assert of_pixels <= mro.MAX_FLAGGED_OF_PIXELS and of_covered <= mro.MAX_FLAGGED_OF_COVERED


def _np(t):
    return t.reshape(-1).cpu().numpy().astype(np.float64)


# ---- 1. a pinhole: the ray cast agrees with the rasteriser ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PINHOLE)
def test_pinhole_ray_cast_agrees_with_the_rasteriser(gpu, bunny, name):
    (v, f), world, r_pin, r_cam = bunny
    view = VIEWS[name]
    cam = _camera(view, gpu)
    color_c, depth_c = r_cam.render_camera(cam, with_color=True)
    color_r, depth_r = r_pin.render_camera(cam, with_color=True)
    H, W = view["H"], view["W"]
    assert depth_c.shape == (H, W, 1) and depth_c.dtype == torch.float32 and color_c.shape == (H, W, 3) and color_c.dtype == torch.uint8
    none, depth_only = r_cam.render_camera(cam)
    assert none is None and torch.equal(depth_only, depth_c)   # the depth does not depend on whether the colour is asked for
    _, z, tri, edge, ff = _oracle(cam, view, world, f)
    _, amb, _ = mo.raster_depth(v, f, model_view(view["c2w"].reshape(-1).tolist(), object_pose(r_pin.config)), view["fx"], view["fy"], view["cx"],
                                view["cy"], H, W)
    flag = (edge < EPS) | amb.reshape(-1)   # a ray near an edge for the ray cast, or a centre near an edge for the raster's own rule
    zc, zr = _np(depth_c), _np(depth_r)
    cov = z > 0
    _check_caps(name, flag, cov)
    ok = ~flag
    differ = ((zc > 0) != (zr > 0)) & ok
    print(f"{name}: coverage differs on {int(((zc > 0) != (zr > 0)).sum())} pixels, {int(differ.sum())} of them off the flags")
    assert not differ.any()
    assert not (((zc > 0) != cov) & ok).any()
    both = ok & cov
    err_c, err_r = (np.abs(zc - z)[both] / z[both]).max(), (np.abs(zr - z)[both] / z[both]).max()
    dz = (np.abs(zc - zr)[both] / z[both]).max()
    print(f"{name}: relative z error against the float64 oracle: ray cast {err_c:.3e}, raster {err_r:.3e}; between the two {dz:.3e} (Z_RTOL {Z_RTOL:g})")
    assert err_c <= Z_RTOL and err_r <= Z_RTOL and dz <= Z_RTOL
    dc = (color_c.reshape(-1, 3).cpu().numpy().astype(int) - color_r.reshape(-1, 3).cpu().numpy().astype(int))
    print(f"{name}: colours differ by at most {np.abs(dc)[ok].max()} of 255 off the flags ({int((np.abs(dc).max(1) > 0)[ok].sum())} pixels differ at all)")
    assert np.abs(dc)[ok].max() <= 1
    assert len(np.unique(color_c.reshape(-1, 3).cpu().numpy()[cov], axis=0)) > 100   # the vertex colours are in the picture
    assert (color_c.reshape(-1, 3).cpu().numpy()[~cov & ok] == 255).all()            # the background elsewhere


# ---- 2, 3. every lens against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LENSES)
def test_every_lens_against_the_oracle(gpu, bunny, name):
    (v, f), world, r_pin, r_cam = bunny
    view = VIEWS[name]
    cam = _camera(view, gpu)
    _, depth = r_cam.render_camera(cam)
    _, z, tri, edge, ff = _oracle(cam, view, world, f)
    flag, cov, got = edge < EPS, z > 0, _np(depth)
    _check_caps(name, flag, cov)
    ok = ~flag
    assert not (((got > 0) != cov) & ok).any(), f"{int((((got > 0) != cov) & ok).sum())} rays differ in coverage off the flags"
    both = ok & cov
    err = (np.abs(got - z)[both] / z[both]).max()
    print(f"{name}: relative z error against the float64 oracle {err:.3e} (Z_RTOL {Z_RTOL:g}); {int((ff <= 0).sum())} rays point backwards")
    assert err <= Z_RTOL
    assert (got[ff <= 0] == 0).all()
    if name.startswith("equirect"):
        # the mesh straddles the plane through the camera: rays with f <= 0 do hit it, and draw nothing
        zb, _, _, _ = mro.cast(*[t.cpu().numpy() for t in (cam.generate_rays(0).origins, cam.generate_rays(0).directions)],
                               -mro.forward_of(view["c2w"]), world, f)
        assert ((zb > 0) & (ff < 0)).sum() > 1000 and (ff <= 0).mean() > 0.4
    again = r_cam.render_camera(cam)[1]
    assert torch.equal(again, depth)   # no atomics: bit-identical run to run
    # the caller's bundle is what is cast: the same picture from the bundle the generator has already made (with nears / fars)
    from signerf_amd.cameras import SceneBox

    bundle = cam.generate_rays(0, aabb_box=SceneBox(torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])))
    assert torch.equal(r_cam.render_camera(cam, ray_bundle=bundle)[1], depth)


# ---- 4. the lens matters --------------------------------------------------------------------------------------------------------------
def test_the_lens_matters_for_a_distorted_camera(gpu, bunny):
    (v, f), world, r_pin, r_cam = bunny
    view = VIEWS["opencv_2_640x480"]
    cam = _camera(view, gpu)
    _, cast = r_cam.render_camera(cam)
    _, raster = r_pin.render_camera(cam)
    _, z, tri, edge, ff = _oracle(cam, view, world, f)
    flagged = int((edge < EPS).sum())
    differ = int(((cast > 0) != (raster > 0)).sum())
    print(f"opencv_2_640x480: the ray cast and the pinhole raster differ in coverage on {differ} pixels; {flagged} are flagged")
    assert differ > flagged and differ > 1000   # k1 = -0.2 moves the outline by pixels


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def test_render_camera_end_to_end_on_a_distorted_camera(gpu, bunny):
    (v, f), world, r_pin, r_cam = bunny
    cfg = small_config(num_proposal_iterations=0, num_nerf_samples_per_ray=32)
    model, _ = make_model(cfg, gpu, density_bias=5.0)
    view = dict(VIEWS["opencv_2_640x480"], fx=155.0, fy=155.0, cx=80.0, cy=60.0, W=160, H=120)
    cam = _camera(view, gpu)
    bundle = cam.generate_rays(0, aabb_box=model.render_aabb)
    depth = model.eval().get_outputs_for_camera_ray_bundle(bundle)["depth"]
    model.train()
    # shape mode
    gen = DatasetGeneratorConfig(masking_mode="shape", mask_dialation=(11, 11), renderer=r_cam.config)
    rgb, mask, cond = render_camera(gen, model, cam, renderer=r_cam)
    _, md = r_cam.render_camera(cam)
    wm, wc = shape_mask_and_condition(md, depth, gen.mask_dialation)
    assert torch.equal(mask, wm) and _same_bits(cond, wc) and mask.any() and not mask.all()
    assert int(((md > 0) & (md < depth)).sum()) > 50
    # aabb + combine_shape_with_depth
    gen = DatasetGeneratorConfig(combine_shape_with_depth=True, mask_dialation=(11, 11), renderer=r_cam.config)
    rgb2, mask, cond = render_camera(gen, model, cam, renderer=r_cam)
    mc, md2 = r_cam.render_camera(cam, with_color=True)
    aabb = torch.tensor([gen.aabb_min, gen.aabb_max], dtype=torch.float32)
    wm, wc = aabb_mask_and_condition_combined(depth, bundle.origins, bundle.directions, aabb, md2, mc, gen.mask_dialation)
    assert torch.equal(md2, md) and torch.equal(rgb, rgb2)
    assert torch.equal(mask, wm) and _same_bits(cond, wc) and mask.any()
    # the pinhole renderer gives this camera another mask: the two modes are not the same path
    _, mask_pin, _ = render_camera(DatasetGeneratorConfig(masking_mode="shape", mask_dialation=(11, 11)), model, cam, renderer=r_pin)
    assert not torch.equal(mask_pin, render_camera(DatasetGeneratorConfig(masking_mode="shape", mask_dialation=(11, 11)), model, cam, renderer=r_cam)[1])


def test_pinhole_lens_is_the_renderer_that_never_heard_of_the_field(gpu, bunny):
    (v, f), world, r_pin, r_cam = bunny
    plain = RendererConfig(scale=mro.BUNNY_SCALE, object_path=r_pin.object_path)
    assert plain == r_pin.config and plain.lens == "pinhole"
    legacy = Renderer(plain, device=gpu)
    legacy.setup()
    assert legacy._host_accel is None and not legacy._uploaded_accel
    for name in ("pinhole_1_531x397", "opencv_2_640x480"):
        cam = _camera(VIEWS[name], gpu)
        c0, d0 = legacy.render_camera(cam, with_color=True)
        c1, d1 = r_pin.render_camera(cam, with_color=True, ray_bundle=cam.generate_rays(0))   # (a bundle is ignored by the pinhole raster)
        assert torch.equal(c0, c1) and torch.equal(d0, d1) and torch.equal(legacy.render_camera(cam)[1], d0)


def test_generate_dataset_with_the_camera_lens(gpu, bunny, tmp_path):
    (v, f), world, r_pin, r_cam = bunny
    from signerf_amd import random_sphere_poses, scene

    size = 64
    model, _ = make_model(small_config(num_proposal_samples_per_ray=(64, 32), num_nerf_samples_per_ray=24), gpu, density_bias=5.0)
    ref = scene.benchmark_cameras(8)[:, :3]
    torch.manual_seed(1)
    syn = random_sphere_poses(3, torch.device("cpu"), 0.5, (30.0, 120.0), (0.0, 360.0), [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])[:, :3]
    trees = {}
    for lens in ("camera", "pinhole"):
        c = DatasetGeneratorConfig(path=tmp_path, dataset_name=lens, fx=1.2 * size, fy=1.2 * size, cx=size / 2, cy=size / 2, width=size, height=size,
                                   rows=3, cols=3, mask_dialation=(7, 7), masking_mode="shape",
                                   renderer=RendererConfig(scale=mro.BUNNY_SCALE, object_path=r_pin.object_path, lens=lens))
        g = DatasetGenerator(c, torch.eye(4)[:3], 1.0, None, device=gpu)
        g.generate_dataset(model, ref, synthetic_camera_to_worlds=syn)
        assert (g.renderer._host_accel is not None) == (lens == "camera")
        trees[lens] = {os.path.relpath(os.path.join(d, fn), tmp_path / lens) for d, _, files in os.walk(tmp_path / lens) for fn in files}
    assert trees["camera"] == trees["pinhole"] and len(trees["camera"]) > 8 * (8 + 3)
    import yaml
    from PIL import Image

    assert yaml.safe_load((tmp_path / "camera" / "config.yml").read_text())["renderer"]["lens"] == "camera"
    assert json.load(open(tmp_path / "camera" / "transforms.json"))["generated_indices"] == list(range(8, 11))
    # these cameras are pinholes: the two lenses draw the same masks up to the pixels on the outline
    n_set = n_diff = 0
    for k in sorted(trees["camera"]):
        if k.startswith("masks/"):
            a, b = (np.asarray(Image.open(tmp_path / lens / k)) > 0 for lens in ("camera", "pinhole"))
            n_set += int(a.sum())
            n_diff += int((a != b).sum())
    assert n_set > 1000 and n_diff <= 0.01 * n_set, (n_set, n_diff)


# ---- 6. misuse --------------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_without_a_launch(gpu, bunny):
    (v, f), world, r_pin, r_cam = bunny
    cam = _camera(VIEWS["fisheye_4_512"], gpu)
    fresh = Renderer(r_cam.config, device=gpu)
    with pytest.raises(RuntimeError, match="setup"):
        fresh.render_camera(cam)
    # set up as a pinhole, switched afterwards: there is no acceleration structure to cast against
    switched = Renderer(RendererConfig(scale=mro.BUNNY_SCALE, object_path=r_pin.object_path), device=gpu)
    switched.setup()
    switched.config.lens = "camera"
    with pytest.raises(RuntimeError, match="acceleration"):
        switched.render_camera(cam)
    small = _camera(dict(VIEWS["fisheye_4_512"], W=64, H=64), gpu).generate_rays(0)
    with pytest.raises(ValueError, match="4096 origins"):
        r_cam.render_camera(cam, ray_bundle=small)
    # the C entry point: a NULL blob, a blob of the wrong size, a struct_size of 0 -- SN_ERR_INVALID with its text, nothing launched
    lib = _lib.load()
    b = cam.generate_rays(0)
    accel = r_cam.accel_on(gpu)
    depth = torch.full((512, 512, 1), 7.0, device=gpu)
    import ctypes as C

    fwd = (C.c_float * 3)(*mro.forward_of(VIEWS["fisheye_4_512"]["c2w"]).tolist())

    def call(accel_ptr, nbytes, opts):
        return lib.sn_mesh_cast_rays(b.origins.data_ptr(), b.directions.data_ptr(), 512, 512, fwd, accel_ptr, nbytes, None, f.shape[0], None, 0,
                                     C.byref(opts), None, depth.data_ptr(), None, _lib.current_stream())

    good = _lib.SnMeshRaysOpts()
    good.znear, good.zfar = 1e-4, 10.0
    zero = _lib.SnMeshRaysOpts()
    zero.znear, zero.zfar, zero.struct_size = 1e-4, 10.0, 0
    assert call(None, accel.numel(), good) == _lib.SN_ERR_INVALID
    assert call(accel.data_ptr(), accel.numel() - 48, good) == _lib.SN_ERR_INVALID and b"sn_mesh_accel_bytes" in lib.sn_last_error(None)
    assert call(accel.data_ptr(), accel.numel(), zero) == _lib.SN_ERR_INVALID and b"struct_size" in lib.sn_last_error(None)
    torch.cuda.synchronize()
    assert (depth == 7.0).all()   # nothing ran
    assert call(accel.data_ptr(), accel.numel(), good) == _lib.SN_OK
    torch.cuda.synchronize()
    assert torch.equal(depth, r_cam.render_camera(cam)[1])
    # a blob that is not one (zeros: no magic number) draws nothing and reads nothing outside itself
    _, d0 = cast_rays(b.origins, b.directions, (0.0, 0.0, -1.0), torch.zeros_like(accel), f.shape[0], 512, 512)
    assert not d0.any()
