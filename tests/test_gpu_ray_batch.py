"""Rays of many cameras in one launch (``sn_generate_ray_batch``, include/signerf_hip_ray_batch.h): tensor ``camera_indices`` in
``Cameras.generate_rays``, ``RayGenerator`` / ``generate_rays_from_indices`` with the pixel gather, and the in-process datamanager.

The criterion is BIT IDENTITY with the per-camera kernel (``sn_generate_rays_camera``), which tests/test_gpu_cameras.py pins against the
oracle: the two kernels call one copy of the arithmetic (csrc/sn_stage.h::sn_camera_ray), so every comparison here is ``torch.equal``."""
import math

import pytest
import torch

from helpers import make_model, small_config
from signerf_amd import (Cameras, CameraType, OrientedBox, PatchPixelSampler, RayGenerator, SceneBox, SIGNeRFDataManager,
                         SIGNeRFDataManagerConfig, scene)
from test_gpu_cameras import DISTORTIONS

pytestmark = pytest.mark.gpu

SIZES = [(40, 56), (40, 56), (33, 17), (33, 17), (24, 40)]   # (H, W) per camera
FIELDS = ("origins", "directions", "pixel_area", "nears", "fars")


def _five(gpu, **kw):
    """PERSPECTIVE plain / distorted, FISHEYE plain / distorted, EQUIRECTANGULAR: three image sizes, per-camera intrinsics."""
    c2w = scene.benchmark_cameras(8)[:5, :3]
    H = torch.tensor([s[0] for s in SIZES])
    W = torch.tensor([s[1] for s in SIZES])
    fx, fy, cx, cy = 0.9 * W, 0.95 * W, W / 2 + 0.25, H / 2 - 0.5
    fx[4], fy[4] = float(H[4]), float(H[4])
    dist = torch.zeros(5, 6)
    dist[1] = torch.tensor(DISTORTIONS[1])
    dist[3] = torch.tensor(DISTORTIONS[1])
    dist[4] = torch.tensor(DISTORTIONS[0])   # (ignored: EQUIRECTANGULAR is never un-distorted)
    types = [CameraType.PERSPECTIVE, CameraType.PERSPECTIVE, CameraType.FISHEYE, CameraType.FISHEYE, CameraType.EQUIRECTANGULAR]
    return Cameras(c2w, fx, fy, cx, cy, W, H, distortion_params=dist, camera_type=types, **kw).to(gpu)


def _equal_size(gpu, B=4, H=24, W=40):
    c2w = scene.benchmark_cameras(8)[:B, :3]
    fx = torch.linspace(30.0, 36.0, B)
    dist = torch.zeros(B, 6)
    dist[1] = torch.tensor(DISTORTIONS[0])
    return Cameras(c2w, fx, fx + 1.0, W / 2 + 0.25, H / 2 - 0.5, W, H, distortion_params=dist).to(gpu)


BOX = SceneBox(aabb=torch.tensor([[-0.3, -0.25, -0.2], [0.3, 0.35, 0.4]]))
OBB = OrientedBox(R=torch.tensor([[math.cos(0.4), -math.sin(0.4), 0.0], [math.sin(0.4), math.cos(0.4), 0.0], [0.0, 0.0, 1.0]]),
                  T=torch.tensor([0.05, -0.02, 0.1]), S=torch.tensor([0.5, 0.6, 0.7]))


def _random_batch(gpu, n, seed, fractional=True):
    """n random (camera, y, x) over the five cameras: every wave mixes them.  Integer triplets or cameras + fractional coords."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, 5, (n,), generator=g)
    hw = torch.tensor(SIZES, dtype=torch.float32)[c]
    if fractional:
        coords = torch.rand(n, 2, generator=g) * hw
        return c.to(gpu), coords.to(gpu)
    yx = torch.floor(torch.rand(n, 2, generator=g) * hw).long()
    return torch.cat([c[:, None], yx], dim=1).to(gpu)


def _over_255(u8):
    """uint8 / 255 as an IEEE fp32 division, which is what the kernel writes and what the reference's CPU image loading gives.  Taken
    on the CPU: on a GPU tensor torch evaluates ``t / 255`` with a Python scalar as ``t * fl(1 / 255)``, which differs from the division
    in the last bit for 126 of the 256 uint8 values, so that expression is no reference for a division."""
    return (u8.cpu().float() / 255).to(u8.device)


def _assert_matches_per_camera(cams, bundle, c, coords, **kw):
    """For every camera b: the rays with c == b equal cams[b].generate_rays(0, coords=coords[c == b], ...) in every field, bit for bit."""
    for b in range(cams.size):
        sel = c == b
        ref = cams[b].generate_rays(0, coords=coords[sel], **kw)
        for k in FIELDS:
            got, want = getattr(bundle, k), getattr(ref, k)
            assert (got is None) == (want is None), k
            if got is not None:
                assert torch.equal(got[sel], want), (b, k, int(sel.sum()))
        assert torch.equal(bundle.metadata["directions_norm"][sel], ref.metadata["directions_norm"]), b
    assert torch.equal(bundle.camera_indices[:, 0], c)


@pytest.mark.parametrize("n", [1, 63, 257, 4097])
def test_bit_identical_to_the_per_camera_kernel(gpu, n):
    """(On the parent commit: NotImplementedError, only integer camera_indices are supported.)"""
    cams = _five(gpu)
    c, coords = _random_batch(gpu, n, seed=n)
    bundle = cams.generate_rays(camera_indices=c[:, None], coords=coords, aabb_box=BOX)
    assert bundle.origins.shape == (n, 3) and bundle.pixel_area.shape == (n, 1) and bundle.nears.shape == (n, 1)
    _assert_matches_per_camera(cams, bundle, c, coords, aabb_box=BOX)
    if n > 1:
        assert len(torch.unique(c[:64])) > 1   # a wave mixes cameras
    # camera_indices [n] instead of [n, 1]
    flat = cams.generate_rays(camera_indices=c, coords=coords, aabb_box=BOX)
    for k in FIELDS:
        assert torch.equal(getattr(flat, k), getattr(bundle, k))
    # the [N, 3] form: pixel centres
    tri = _random_batch(gpu, n, seed=100 + n, fractional=False)
    b3, pixels = cams.generate_rays_from_indices(tri, aabb_box=BOX)
    assert pixels is None
    _assert_matches_per_camera(cams, b3, tri[:, 0], tri[:, 1:].float() + 0.5, aabb_box=BOX)
    gen = RayGenerator(cams, aabb_box=BOX)(tri)
    for k in FIELDS:
        assert torch.equal(getattr(gen, k), getattr(b3, k))


@pytest.mark.parametrize("n", [257, 4097])
def test_bit_identical_without_distortion_and_with_an_obb(gpu, n):
    cams = _five(gpu)
    c, coords = _random_batch(gpu, n, seed=7 * n)
    plain = cams.generate_rays(camera_indices=c[:, None], coords=coords, aabb_box=BOX, disable_distortion=True)
    _assert_matches_per_camera(cams, plain, c, coords, aabb_box=BOX, disable_distortion=True)
    dist = cams.generate_rays(camera_indices=c[:, None], coords=coords, aabb_box=BOX)
    on_lens = (c == 1) | (c == 3)
    assert not torch.equal(plain.directions[on_lens], dist.directions[on_lens]) and torch.equal(plain.directions[~on_lens], dist.directions[~on_lens])
    obb = cams.generate_rays(camera_indices=c[:, None], coords=coords, obb_box=OBB)
    _assert_matches_per_camera(cams, obb, c, coords, obb_box=OBB)
    assert bool((obb.nears < 1e9).any()) and bool((obb.nears >= 1e10).any())   # hits and misses
    none = cams.generate_rays(camera_indices=c[:, None], coords=coords)
    assert none.nears is None and none.fars is None and torch.equal(none.directions, dist.directions)


def test_order_does_not_matter(gpu):
    """Sorted by camera (every wave sees one record) and shuffled (every lane its own): the same ray per triplet."""
    cams = _five(gpu)
    tri = _random_batch(gpu, 5000, seed=11, fractional=False)
    order = torch.argsort(tri[:, 0], stable=True)
    a, _ = cams.generate_rays_from_indices(tri, aabb_box=BOX)
    s, _ = cams.generate_rays_from_indices(tri[order], aabb_box=BOX)
    assert bool((tri[order][:-1, 0] <= tri[order][1:, 0]).all())
    for k in FIELDS:
        assert torch.equal(getattr(a, k)[order], getattr(s, k)), k
    assert torch.equal(a.metadata["directions_norm"][order], s.metadata["directions_norm"])


def test_shapes(gpu):
    cams = _five(gpu)
    P = 2
    c, coords = _random_batch(gpu, P * 32 * 32, seed=5)
    ci, co = c.reshape(P, 32, 32, 1), coords.reshape(P, 32, 32, 2)
    b = cams.generate_rays(camera_indices=ci, coords=co, aabb_box=BOX)
    assert b.shape == (P, 32, 32) and b.origins.shape == (P, 32, 32, 3) and b.directions.shape == (P, 32, 32, 3)
    assert b.pixel_area.shape == b.nears.shape == b.fars.shape == b.camera_indices.shape == b.metadata["directions_norm"].shape == (P, 32, 32, 1)
    f = cams.generate_rays(camera_indices=ci, coords=co, aabb_box=BOX, keep_shape=False)
    assert f.shape == (P * 1024,) and torch.equal(f.directions, b.directions.reshape(-1, 3)) and f.camera_indices.shape == (P * 1024, 1)
    e = cams.generate_rays(camera_indices=torch.zeros((0, 1), dtype=torch.int64, device=gpu), coords=torch.zeros((0, 2), device=gpu), aabb_box=BOX)
    assert e.origins.shape == (0, 3) and e.directions.shape == (0, 3) and e.pixel_area.shape == (0, 1) and e.nears.shape == (0, 1)
    assert e.fars.shape == (0, 1) and e.camera_indices.shape == (0, 1) and e.metadata["directions_norm"].shape == (0, 1)
    e3, px = cams.generate_rays_from_indices(torch.zeros((0, 3), dtype=torch.int64, device=gpu))
    assert e3.origins.shape == (0, 3) and px is None and e3.nears is None


def test_out_of_range_camera_indices_give_nan_rays(gpu):
    cams = _equal_size(gpu)
    B = cams.size
    images = torch.randint(0, 256, (B, 24, 40, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(gpu)
    g = torch.Generator().manual_seed(2)
    n = 300
    tri = torch.stack([torch.randint(0, B, (n,), generator=g), torch.randint(0, 24, (n,), generator=g), torch.randint(0, 40, (n,), generator=g)], 1)
    bad = torch.zeros(n, dtype=torch.bool)
    bad[[0, 17, 63, 64, 200, n - 1]] = True
    tri_bad = tri.clone()
    tri_bad[bad, 0] = torch.tensor([-1, B, -1, B, 1 << 40, -(1 << 40)])
    good, gpx = cams.generate_rays_from_indices(tri.to(gpu), images=images, aabb_box=BOX)
    got, px = cams.generate_rays_from_indices(tri_bad.to(gpu), images=images, aabb_box=BOX)
    torch.cuda.synchronize()   # HIP reports no error
    bad = bad.to(gpu)
    for k in FIELDS:
        assert bool(torch.isnan(getattr(got, k)[bad]).all()), k
        assert torch.equal(getattr(got, k)[~bad], getattr(good, k)[~bad]), k
    assert bool(torch.isnan(got.metadata["directions_norm"][bad]).all()) and bool(torch.isnan(px[bad]).all())
    assert torch.equal(px[~bad], gpx[~bad]) and not bool(torch.isnan(gpx).any())
    assert torch.equal(got.camera_indices[:, 0], tri_bad[:, 0].to(gpu))   # the given ones
    # the coords form
    c = tri_bad[:, 0].to(gpu)
    coords = tri[:, 1:].float().to(gpu) + 0.5
    b2 = cams.generate_rays(camera_indices=c, coords=coords, aabb_box=BOX)
    torch.cuda.synchronize()
    for k in FIELDS:
        assert bool(torch.isnan(getattr(b2, k)[bad]).all()) and torch.equal(getattr(b2, k)[~bad], getattr(good, k)[~bad]), k


@pytest.mark.parametrize("channels", [3, 4, 1])
def test_pixels(gpu, channels):
    cams = _equal_size(gpu)
    B, H, W = cams.size, 24, 40
    images = torch.randint(0, 256, (B, H, W, channels), dtype=torch.uint8, generator=torch.Generator().manual_seed(channels)).to(gpu)
    g = torch.Generator().manual_seed(9)
    n = 1500
    tri = torch.stack([torch.randint(0, B, (n,), generator=g), torch.randint(0, H, (n,), generator=g), torch.randint(0, W, (n,), generator=g)], 1).to(gpu)
    bundle, pixels = RayGenerator(cams, images=images)(tri)
    assert pixels.shape == (n, channels) and pixels.dtype == torch.float32
    assert torch.equal(pixels, _over_255(images[tri[:, 0], tri[:, 1], tri[:, 2]]))
    assert len(torch.unique(pixels)) > 200   # (every uint8 value / 255 is compared: the division is IEEE)
    _assert_matches_per_camera(cams, bundle, tri[:, 0], tri[:, 1:].float() + 0.5)
    # (y, x) outside the image: NaN pixels, a finite ray (coordinates outside the image are legal for rays)
    out = tri.clone()
    where = torch.tensor([3, 64, 700, n - 1], device=gpu)
    out[where, 1:] = torch.tensor([[H, 0], [-1, 5], [2, W], [3, -1]], device=gpu)
    b2, p2 = cams.generate_rays_from_indices(out, images=images)
    torch.cuda.synchronize()
    mask = torch.zeros(n, dtype=torch.bool, device=gpu)
    mask[where] = True
    assert bool(torch.isnan(p2[mask]).all()) and torch.equal(p2[~mask], pixels[~mask])
    assert bool(torch.isfinite(b2.directions).all()) and bool(torch.isfinite(b2.pixel_area).all())
    _assert_matches_per_camera(cams, b2, out[:, 0], out[:, 1:].float() + 0.5)


def test_times_and_metadata_are_gathered_per_ray(gpu):
    times = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])
    meta = {"exposure": torch.arange(10.0).reshape(5, 2), "name": "five"}
    cams = _five(gpu, times=times, metadata=meta)
    c, coords = _random_batch(gpu, 513, seed=3)
    b = cams.generate_rays(camera_indices=c.reshape(27, 19, 1), coords=coords.reshape(27, 19, 2))
    assert torch.equal(b.times, times.to(gpu)[c].reshape(27, 19, 1))
    assert torch.equal(b.metadata["exposure"], meta["exposure"].to(gpu)[c].reshape(27, 19, 2))
    assert "name" not in b.metadata and b.metadata["directions_norm"].shape == (27, 19, 1)


def test_a_million_rays_in_one_call(gpu):
    cams = _five(gpu)
    n = (1 << 20) + 3
    c, coords = _random_batch(gpu, n, seed=21)
    bundle = cams.generate_rays(camera_indices=c, coords=coords, aabb_box=BOX)
    pick = torch.cat([torch.arange(0, n - 3, (n - 3) // 4096, device=gpu)[:4096], torch.arange(n - 3, n, device=gpu)])
    assert pick.numel() == 4099
    sub = bundle._map(lambda t: t[pick])
    _assert_matches_per_camera(cams, sub, c[pick], coords[pick], aabb_box=BOX)


def test_rescale_rebuilds_the_camera_table(gpu):
    cams = _five(gpu)
    c, coords = _random_batch(gpu, 300, seed=4)
    before = cams.generate_rays(camera_indices=c, coords=coords)
    cams.rescale_output_resolution(0.5)
    after = cams.generate_rays(camera_indices=c, coords=coords)
    assert not torch.equal(before.directions, after.directions)
    _assert_matches_per_camera(cams, after, c, coords)


def test_next_train_end_to_end(gpu):
    """Patches of 32 x 32 across a small dataset, rendered flat; the same triplets generated per camera with the existing path and
    rendered give the same rgb, bit for bit."""
    cfg = small_config()
    model, _ = make_model(cfg, gpu)
    B, H, W = 3, 40, 48
    c2w = scene.benchmark_cameras(8)[:B, :3]
    cams = Cameras(c2w, 50.0, 50.0, W / 2, H / 2, W, H).to(gpu)
    images = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(gpu)
    box = SceneBox(aabb=torch.tensor([[-0.4, -0.4, -0.4], [0.4, 0.4, 0.4]]))
    gen = torch.Generator(device=gpu).manual_seed(5)
    dm = SIGNeRFDataManager(SIGNeRFDataManagerConfig(train_num_rays_per_batch=2048 + 100, patch_size=32), cams, images, aabb_box=box, generator=gen)
    assert isinstance(dm.train_pixel_sampler, PatchPixelSampler) and dm.get_train_rays_per_batch() == 2048
    bundle, batch = dm.next_train(0)
    R = 2048
    idx = batch["indices"]
    assert len(bundle) == R and bundle.origins.shape == (R, 3) and idx.shape == (R, 3) and batch["image"].shape == (R, 3)
    assert torch.equal(batch["image"], _over_255(images[idx[:, 0], idx[:, 1], idx[:, 2]]))
    patches = idx.reshape(2, 32, 32, 3)
    for p in patches:   # a contiguous 32 x 32 block of one image
        assert len(torch.unique(p[..., 0])) == 1
        y0, x0 = int(p[0, 0, 1]), int(p[0, 0, 2])
        ys, xs = torch.meshgrid(torch.arange(32, device=gpu), torch.arange(32, device=gpu), indexing="ij")
        assert torch.equal(p[..., 1], ys + y0) and torch.equal(p[..., 2], xs + x0) and 0 <= y0 <= H - 32 and 0 <= x0 <= W - 32
    rgb = model.get_outputs(bundle)["rgb"]
    assert rgb.shape == (R, 3) and bool(torch.isfinite(rgb).all()) and float(rgb.std()) > 0
    for b in range(B):
        sel = idx[:, 0] == b
        if not bool(sel.any()):
            continue
        ref = cams[b].generate_rays(0, coords=idx[sel][:, 1:].float() + 0.5, aabb_box=box)
        assert torch.equal(ref.directions, bundle.directions[sel]) and torch.equal(ref.nears, bundle.nears[sel])
        assert torch.equal(model.get_outputs(ref)["rgb"], rgb[sel]), b
    assert dm.train_count == 1
