"""Ray batches across cameras, CPU side: the companion C header include/signerf_hip_ray_batch.h against the binding and the library's
exports, the argument checks of ``sn_generate_ray_batch`` (in a child process: nothing is launched), the pixel samplers of
signerf_amd/data.py on ``device="cpu"`` and the host-side argument errors of ``Cameras.generate_rays``.  No GPU."""

import pytest
import torch

from abi_helpers import c99_probe, refusal_sweep
from signerf_amd import Cameras, CameraType, PatchPixelSampler, PatchPixelSamplerConfig, PixelSampler, PixelSamplerConfig, _lib


# ---- the companion C header ------------------------------------------------------------------------------------------------------------
def test_ray_batch_header_binding_and_exports_agree(built_lib):
    """(The header against the binding, the exports and build.HEADERS: tests/test_cabi.py, for every header.)"""
    assert sorted(_lib.header("ray_batch").functions) == ["sn_generate_ray_batch", "sn_ray_batch_abi_version"]
    lib = _lib.load()
    assert lib.sn_ray_batch_abi_version() == _lib.header("ray_batch").version == 1
    assert b"sn_ray_batch_kernel" in open(built_lib, "rb").read()


def test_camera_record_is_26_dwords(tmp_path):
    """The device camera table is built as [B, 26] int32 rows (cameras.py::_camera_table): the C struct must be exactly that."""
    import ctypes as C

    got = [int(x) for x in c99_probe(tmp_path, "signerf_hip_ray_batch.h", "%zu %zu %zu %zu %zu %zu %zu %d",
                                     "sizeof(SnCameraDesc), offsetof(SnCameraDesc, fx), offsetof(SnCameraDesc, height), "
                                     "offsetof(SnCameraDesc, width), offsetof(SnCameraDesc, camera_type), "
                                     "offsetof(SnCameraDesc, has_distortion), offsetof(SnCameraDesc, distortion), SN_RAY_BATCH_ABI_VERSION")]
    d = _lib.SnCameraDesc
    assert got == [104, 48, 64, 68, 72, 76, 80, 1]
    assert got[:7] == [C.sizeof(d), d.fx.offset, d.height.offset, d.width.offset, d.camera_type.offset, d.has_distortion.offset, d.distortion.offset]


_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
fake = 0x1000   # never dereferenced: every call below is refused (or n == 0) before the device is touched
box = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
def call(cams=fake, ncam=3, tri=fake, cidx=N, coords=N, n=16, out=fake, aabb=None, images=N, h=0, w=0, c=0, pixels=N):
    st = lib.sn_generate_ray_batch(cams, ncam, tri, cidx, coords, n, out, out, out, out, aabb, N, N, images, h, w, c, pixels, N)
    msg = lib.sn_last_error(None)
    return "%d:%s" % (st, "text" if (st == 0 or (msg and b"sn_generate_ray_batch" in msg)) else "notext")
calls = {
 "abi": lambda: "%d:text" % lib.sn_ray_batch_abi_version(),
 "all_null": lambda: call(cams=N, tri=N, out=N),
 "no_cameras": lambda: call(cams=N),
 "zero_cameras": lambda: call(ncam=0),
 "negative_n": lambda: call(n=-1),
 "both_forms": lambda: call(cidx=fake, coords=fake),
 "both_forms_half": lambda: call(coords=fake),
 "neither_form": lambda: call(tri=N),
 "cidx_without_coords": lambda: call(tri=N, cidx=fake),
 "coords_without_cidx": lambda: call(tri=N, coords=fake),
 "img_c_5": lambda: call(images=fake, h=8, w=8, c=5, pixels=fake),
 "img_c_0": lambda: call(images=fake, h=8, w=8, c=0, pixels=fake),
 "img_h_0": lambda: call(images=fake, h=0, w=8, c=3, pixels=fake),
 "images_without_pixels": lambda: call(images=fake, h=8, w=8, c=3),
 "pixels_without_images": lambda: call(pixels=fake),
 "pixels_with_coords_form": lambda: call(tri=N, cidx=fake, coords=fake, images=fake, h=8, w=8, c=3, pixels=fake),
 "n_0_is_ok": lambda: call(n=0),
 "n_0_coords_form_is_ok": lambda: call(tri=N, cidx=fake, coords=fake, n=0, aabb=box),
}
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_generate_ray_batch_refuses_bad_arguments_before_the_device(built_lib):
    """NULL mandatory pointers, both index forms together, neither, img_c = 5, pixels with the coords form, ...: SN_ERR_INVALID with text in
    sn_last_error, in a child process -- nothing is launched (n = 0 is SN_OK without a launch), and a crash would be a segfault."""
    got = refusal_sweep(_SWEEP)
    want = {k: "1:text" for k in got}
    want.update({"abi": "1:text", "n_0_is_ok": "0:text", "n_0_coords_form_is_ok": "0:text"})
    assert len(got) == 18 and got == want


# ---- the samplers ----------------------------------------------------------------------------------------------------------------------
def test_patch_sampler_equals_the_formula_from_the_same_seed():
    ps, B, H, W, bs = 8, 5, 37, 53, 8 * 8 * 6 + 13
    sampler = PatchPixelSamplerConfig().setup(patch_size=ps, num_rays_per_batch=bs, generator=torch.Generator().manual_seed(42))
    assert isinstance(sampler, PatchPixelSampler) and sampler.num_rays_per_batch == 8 * 8 * 6
    got = sampler.sample_method(sampler.num_rays_per_batch, B, H, W)
    # signerf/data/signerf_patch_pixel_sampler.py's expression, from the same seed
    g = torch.Generator().manual_seed(42)
    sub_bs = sampler.num_rays_per_batch // ps**2
    idx = torch.rand((sub_bs, 3), generator=g) * torch.tensor([B, H - ps, W - ps])
    idx = idx.view(sub_bs, 1, 1, 3).broadcast_to(sub_bs, ps, ps, 3).clone()
    yys, xxs = torch.meshgrid(torch.arange(ps), torch.arange(ps), indexing="ij")
    idx[:, ..., 1] += yys
    idx[:, ..., 2] += xxs
    want = torch.floor(idx).long().flatten(0, 2)
    assert got.dtype == torch.int64 and got.shape == (sub_bs * ps * ps, 3) and torch.equal(got, want)
    # every patch: a contiguous ps x ps block of one image, inside its bounds
    for p in got.reshape(sub_bs, ps, ps, 3):
        assert len(torch.unique(p[..., 0])) == 1 and 0 <= int(p[0, 0, 0]) < B
        y0, x0 = int(p[0, 0, 1]), int(p[0, 0, 2])
        assert 0 <= y0 <= H - ps and 0 <= x0 <= W - ps
        assert torch.equal(p[..., 1], yys + y0) and torch.equal(p[..., 2], xxs + x0)
    assert len(torch.unique(got[:, 0])) > 1
    # the second draw continues the generator's stream
    assert not torch.equal(sampler.sample_method(sampler.num_rays_per_batch, B, H, W), got)


def test_patch_sampler_rounds_the_batch_down():
    s = PatchPixelSampler(PatchPixelSamplerConfig(patch_size=32))
    assert s.config.patch_size == 32 and s.num_rays_per_batch == 4096
    s.set_num_rays_per_batch(4096 + 100)
    assert s.num_rays_per_batch == 4096
    s.set_num_rays_per_batch(1023)
    assert s.num_rays_per_batch == 0
    with pytest.raises(ValueError, match="does not fit"):
        s.sample_method(1024, 2, 31, 64)
    with pytest.raises(TypeError, match="no field"):
        PixelSamplerConfig().setup(patch_size=4)


@pytest.mark.parametrize("cls,cfg", [(PixelSampler, PixelSamplerConfig()), (PatchPixelSampler, PatchPixelSamplerConfig(patch_size=4))])
def test_with_a_mask_only_masked_pixels_are_drawn(cls, cfg):
    """(The patch sampler reduces to the base sampler under a mask, as the reference's does.)"""
    B, H, W = 3, 9, 11
    mask = torch.zeros(B, H, W, 1)
    mask[0, 2, 3] = mask[0, 8, 10] = mask[2, 0, 0] = mask[2, 4, 5] = 1
    s = cls(cfg, generator=torch.Generator().manual_seed(1))
    got = s.sample_method(512, B, H, W, mask=mask)
    assert got.shape == (512, 3) and bool((mask[got[:, 0], got[:, 1], got[:, 2], 0] == 1).all())
    assert {tuple(r) for r in got.tolist()} == {(0, 2, 3), (0, 8, 10), (2, 0, 0), (2, 4, 5)}   # each of the four is drawn
    counts = torch.unique(got[:, 0] * 1000 + got[:, 1] * 20 + got[:, 2], return_counts=True)[1]
    assert int(counts.min()) > 80   # uniform: 128 expected each, sd < 10
    ignoring = cls(type(cfg)(**{**cfg.__dict__, "ignore_mask": True}), generator=torch.Generator().manual_seed(1))
    free = ignoring.sample_method(512, B, H, W, mask=mask)
    assert not bool((mask[free[:, 0], free[:, 1], free[:, 2], 0] == 1).all())


def test_base_sampler_stays_inside_and_collates():
    B, H, W = 4, 7, 13
    s = PixelSampler(PixelSamplerConfig(num_rays_per_batch=3000), generator=torch.Generator().manual_seed(0))
    idx = s.sample_method(3000, B, H, W)
    want = torch.floor(torch.rand((3000, 3), generator=torch.Generator().manual_seed(0)) * torch.tensor([B, H, W])).long()
    assert torch.equal(idx, want)
    assert bool((idx >= 0).all()) and bool((idx < torch.tensor([B, H, W])).all())
    assert [len(torch.unique(idx[:, k])) for k in range(3)] == [B, H, W]   # every image, row and column is reached
    image = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    out = s.sample({"image": image, "image_idx": torch.tensor([10, 11, 12, 13])})
    i = out["indices"]
    assert i.shape == (3000, 3) and bool((i[:, 0] >= 10).all()) and out["image"].dtype == torch.float32
    assert torch.equal(out["image"], image[i[:, 0] - 10, i[:, 1], i[:, 2]].float() / 255)
    s.set_num_rays_per_batch(17)
    assert s.sample({"image": image, "image_idx": torch.arange(B)})["indices"].shape == (17, 3)


# ---- argument errors of Cameras.generate_rays: host checks, before the GPU is touched ------------------------------------------------------
def _cams(types=CameraType.PERSPECTIVE):
    c2w = torch.eye(4)[:3].expand(3, 3, 4)
    return Cameras(c2w, 10.0, 10.0, 4.0, 4.0, 8, 8, camera_type=types)


def test_tensor_indices_argument_errors():
    c, coords = torch.tensor([[0], [2]]), torch.zeros(2, 2)
    with pytest.raises(NotImplementedError, match="coords"):
        _cams().generate_rays(camera_indices=c)
    with pytest.raises(NotImplementedError, match="distortion_params_delta"):
        _cams().generate_rays(camera_indices=c, coords=coords, distortion_params_delta=torch.zeros(6))
    with pytest.raises(NotImplementedError, match="camera_opt_to_camera"):
        _cams().generate_rays(camera_indices=c, coords=coords, camera_opt_to_camera=torch.zeros(2, 3, 4))
    # ANY camera of the table with an unsupported type, whether a ray asks for it or not
    mixed = _cams([CameraType.PERSPECTIVE, CameraType.ORTHOPHOTO, CameraType.FISHEYE])
    with pytest.raises(NotImplementedError, match="ORTHOPHOTO"):
        mixed.generate_rays(camera_indices=c, coords=coords)
    with pytest.raises(NotImplementedError, match="ORTHOPHOTO"):
        mixed.generate_rays_from_indices(torch.zeros(4, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="camera_indices"):
        _cams().generate_rays(camera_indices=torch.zeros(3, dtype=torch.int64), coords=coords)
    # after the host checks: the cameras are not on the GPU
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        _cams().generate_rays(camera_indices=c, coords=coords)


def test_camera_table_follows_the_host_mirror():
    """The [B, 26] int32 rows handed to the kernel: the integer path's has_distortion rule, rebuilt by rescale_output_resolution."""
    import ctypes as C

    import numpy as np

    dist = torch.zeros(3, 6)
    dist[1] = torch.tensor([0.1, 0.0, 0.0, 0.0, 0.0, -0.01])
    cams = Cameras(torch.eye(4)[:3].expand(3, 3, 4) * 1.0, torch.tensor([10.0, 11.0, 12.0]), 9.0, 4.0, 5.0, torch.tensor([8, 9, 10]), 7,
                   distortion_params=dist, camera_type=[CameraType.PERSPECTIVE, CameraType.FISHEYE, CameraType.EQUIRECTANGULAR])

    def records(c, disable=False):
        rows = c._host_table(disable)
        assert rows.dtype == torch.int32 and rows.shape == (3, 26) and rows.is_contiguous()
        return (_lib.SnCameraDesc * 3).from_buffer_copy(np.ascontiguousarray(rows.numpy()).tobytes())

    r = records(cams)
    assert [x.fx for x in r] == [10.0, 11.0, 12.0] and [x.width for x in r] == [8, 9, 10] and [x.height for x in r] == [7, 7, 7]
    assert [x.camera_type for x in r] == [1, 2, 3] and [x.has_distortion for x in r] == [0, 1, 0]
    assert list(r[1].distortion) == pytest.approx([0.1, 0, 0, 0, 0, -0.01]) and list(r[0].c2w) == torch.eye(4)[:3].reshape(-1).tolist()
    assert [x.has_distortion for x in records(cams, disable=True)] == [0, 0, 0] and list(records(cams, disable=True)[1].distortion) == [0.0] * 6
    cams._tables[("stale", False)] = None
    cams.rescale_output_resolution(0.5)
    assert cams._tables == {}
    r = records(cams)
    assert [x.fx for x in r] == [5.0, 5.5, 6.0] and [x.width for x in r] == [4, 4, 5] and [x.height for x in r] == [3, 3, 3]
    assert C.sizeof(_lib.SnCameraDesc) == 104
