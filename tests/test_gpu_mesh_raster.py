"""Shape masking mode on the GPU: ``sn_mesh_raster_depth`` against the float64 reference rasteriser (tests/mesh_oracle.py).

Gates: coverage equal except at pixels the oracle marks ambiguous (centre within a normalised 1e-5 of an edge of a possibly-front
triangle, at the near / far plane, or on an edge-on triangle); relative depth error <= 1e-5 where both cover, grazing hits excluded."""
import numpy as np
import pytest
import torch

import mesh_oracle as mo
from signerf_amd import Cameras, scene
from signerf_amd.renderer import Renderer, RendererConfig, model_view, object_pose, raster_depth

pytestmark = pytest.mark.gpu


def _mv(t=(0.0, 0.0, 0.0)):
    return np.hstack([np.eye(3), np.asarray(t, dtype=np.float64).reshape(3, 1)])


def _gpu_depth(gpu, v, f, mv, fx, fy, cx, cy, H, W, cull=True, **kw):
    d = raster_depth(torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), mv, fx, fy, cx, cy, H, W, cull_back_faces=cull, **kw)
    assert d.shape == (H, W, 1) and d.dtype == torch.float32
    return d[..., 0].cpu().numpy().astype(np.float64)


def _compare(got, v, f, mv, fx, fy, cx, cy, H, W, cull=True, min_cover=1, max_amb_frac=0.02, **kw):
    ref, amb, graze = mo.raster_depth(v, f, mv, fx, fy, cx, cy, H, W, cull=cull, **kw)
    cg, cr = got > 0, ref > 0
    bad = (cg != cr) & ~amb
    assert not bad.any(), f"{bad.sum()} pixels differ in coverage away from any edge, e.g. {np.argwhere(bad)[:5].tolist()}"
    assert amb.sum() <= max_amb_frac * max(cr.sum(), 1) + 16, amb.sum()   # the exclusion stays a thin set
    both = cg & cr & ~amb & ~graze
    if both.any():
        rel = np.abs(got[both] - ref[both]) / ref[both]
        assert rel.max() <= 1e-5, rel.max()
    assert cr.sum() >= min_cover
    return ref


CASES = {
    # name: (mesh, mv, fx, fy, cx, cy, H, W, cull, min covered pixels)
    "closed_icosphere": (lambda: mo.icosphere(3), _mv((0.1, -0.05, -3.0)), 100.0, 100.0, 64.0, 48.0, 96, 128, True, 2000),
    "soup_cull": (lambda: mo.triangle_soup(300, seed=1), _mv(), 80.0, 80.0, 64.0, 48.0, 96, 128, True, 1000),
    "soup_both_sides": (lambda: mo.triangle_soup(300, seed=1), _mv(), 80.0, 80.0, 64.0, 48.0, 96, 128, False, 2000),
    "through_znear_and_beyond_zfar": (lambda: mo.triangle_soup(400, seed=2, center=(0.0, 0.0, -5.0), spread=7.0, size=1.5), _mv(),
                                      60.0, 60.0, 48.0, 48.0, 96, 96, False, 1000),
    "camera_inside_sphere_culled": (lambda: mo.icosphere(3, 2.0), _mv(), 60.0, 60.0, 32.0, 32.0, 64, 64, True, 0),
    "camera_inside_sphere_both": (lambda: mo.icosphere(3, 2.0), _mv(), 60.0, 60.0, 32.0, 32.0, 64, 64, False, 64 * 64),
    "full_frame": (lambda: (np.array([[-100, -100, -1.5], [100, -100, -1.0], [0, 100, -1.2]], np.float32), np.array([[0, 1, 2]], np.int32)),
                   _mv(), 50.0, 50.0, 32.0, 32.0, 64, 64, True, 64 * 64),
    "sub_pixel": (lambda: mo.triangle_soup(20000, seed=4, spread=1.0, size=0.002), _mv(), 100.0, 100.0, 48.0, 48.0, 96, 96, False, 1),
    "ragged_97x131": (lambda: mo.icosphere(2), _mv((0.0, 0.0, -2.5)), 110.0, 110.0, 65.5, 48.5, 97, 131, True, 3000),
    "off_centre_fx_ne_fy": (lambda: mo.icosphere(3), _mv((0.2, 0.1, -3.0)), 90.0, 140.0, 40.3, 70.9, 120, 100, True, 1000),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_raster_matches_float64_oracle(gpu, name):
    mesh, mv, fx, fy, cx, cy, H, W, cull, min_cover = CASES[name]
    v, f = mesh()
    got = _gpu_depth(gpu, v, f, mv, fx, fy, cx, cy, H, W, cull)
    ref = _compare(got, v, f, mv, fx, fy, cx, cy, H, W, cull, min_cover)
    if name == "camera_inside_sphere_culled":
        assert not (got > 0).any()
    if name == "through_znear_and_beyond_zfar":
        assert (got[got > 0] <= 10.0).all() and (got[got > 0] >= 1e-4).all()


def test_custom_near_and_far_planes(gpu):
    """A plane sloping from z-depth 0.2 to 6 through znear = 0.5 and zfar = 4: both cuts where the oracle puts them."""
    v = np.array([[-8, -8, -0.2], [8, -8, -6.0], [8, 8, -6.0], [-8, 8, -0.2]], np.float32)
    f = np.array([[0, 2, 1], [0, 3, 2]], np.int32)
    got = _gpu_depth(gpu, v, f, _mv(), 40.0, 40.0, 32.0, 32.0, 64, 64, False, znear=0.5, zfar=4.0)
    _compare(got, v, f, _mv(), 40.0, 40.0, 32.0, 32.0, 64, 64, False, 100, znear=0.5, zfar=4.0)
    cov = got > 0
    assert cov.any() and (~cov).any() and got[cov].min() >= 0.5 and got[cov].max() <= 4.0


def test_million_triangles_and_bit_identical_runs(gpu):
    v, f = mo.icosphere(8, 0.8)   # 1 310 720 triangles, most of them smaller than a pixel at 64 x 64
    mv = _mv((0.05, 0.0, -2.0))
    a = _gpu_depth(gpu, v, f, mv, 70.0, 70.0, 32.0, 32.0, 64, 64)
    _compare(a, v, f, mv, 70.0, 70.0, 32.0, 32.0, 64, 64, True, 500, max_amb_frac=0.1)   # (every triangle is near some centre)
    b = _gpu_depth(gpu, v, f, mv, 70.0, 70.0, 32.0, 32.0, 64, 64)
    assert a.tobytes() == b.tobytes()
    v, f = mo.triangle_soup(2000, seed=9)   # overlapping soup: the front-most pick must not depend on scheduling either
    runs = {_gpu_depth(gpu, v, f, _mv(), 80.0, 80.0, 64.0, 48.0, 96, 128, False).tobytes() for _ in range(3)}
    assert len(runs) == 1


def test_empty_mesh_gives_zeros(gpu):
    d = raster_depth(torch.zeros((0, 3), device=gpu), torch.zeros((0, 3), dtype=torch.int32, device=gpu), _mv(), 10.0, 10.0, 4.0, 4.0, 8, 8,
                     out=torch.full((8, 8, 1), 7.0, device=gpu))
    assert torch.equal(d.cpu(), torch.zeros(8, 8, 1))


def _write_obj(path, v, f):
    with open(path, "w") as fh:
        fh.write("".join(f"v {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in v.tolist()))
        fh.write("".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f.tolist()))


def test_renderer_render_camera_pose_and_no_sync(gpu, tmp_path):
    """Renderer.render_camera: the object pose (position / rotation / scale x 10) and the camera pose composed on the host, the depth on
    the GPU -- against the oracle given the same matrices, and without a device sync once the mesh is on the device."""
    v, f = mo.icosphere(3)
    _write_obj(tmp_path / "ico.obj", v, f)
    cfg = RendererConfig(position=[0.02, -0.03, 0.01], rotation=[20, 40, -30], scale=[0.012, 0.008, 0.01], object_path=str(tmp_path / "ico.obj"))
    r = Renderer(cfg, device=gpu)
    r.setup()
    H, W = 72, 96
    cams = Cameras(scene.benchmark_cameras(8)[:, :3], 90.0, 90.0, W / 2, H / 2, W, H).to(gpu)
    color, _ = r.render_camera(cams[0])   # first view on this device uploads the mesh
    assert color is None
    for k in (1, 5):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            _, depth = r.render_camera(cams[k])
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert depth.shape == (H, W, 1) and depth.device.type == "cuda"
        mv = model_view(cams._host[k, :12].tolist(), object_pose(cfg))
        vv, ff = r._host_mesh
        _compare(depth[..., 0].cpu().numpy().astype(np.float64), vv, ff, mv, 90.0, 90.0, W / 2, H / 2, H, W, True, 100)
