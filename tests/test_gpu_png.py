"""png_encoder="hip" on the GPU: the kernels of signerf_amd/csrc/sn_png.h must write, byte for byte, the file of the serial host reference
encoder (tests/c/png_encode.cpp, built from the shared header sn_png_codes.h) for every image of tests/png_cases.py; then determinism
across streams, the refusals, the size caps and ``GeneratedDataset`` / ``DatasetGenerator`` with "hip" against "native"."""
import io
import json
import os

import numpy as np
import pytest
import torch

import png_cases as pc
from signerf_amd import _lib, dataset_io

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """name -> the host reference encoder's file, computed once per image."""
    exe = pc.build_reference(str(tmp_path_factory.mktemp("png_encode")))
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = pc.reference_png(exe, pc.images()[name])
        return cache[name]

    return get


def encode(u8, gpu):
    return dataset_io.encode_png_hip(torch.from_numpy(np.array(u8)).to(gpu))


@pytest.mark.parametrize("name", pc.NAMES)
def test_device_bytes_equal_the_host_reference(gpu, reference, name):
    u8 = pc.images()[name]
    got, want = encode(u8, gpu), reference(name)
    print(name, u8.shape, "device", len(got), "reference", len(want), "stream", len(pc.filtered_stream(u8)))
    assert len(got) == len(want)
    if got != want:
        first = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        raise AssertionError(f"{name}: first differing byte at {first} of {len(want)}")
    pc.check_file(got, u8)
    assert len(got) <= _lib.load().sn_png_max_file_bytes(*u8.shape)


def test_size_caps(gpu, reference):
    """Caps that keep a broken matcher from passing (the device file IS the reference's, by the test above; both are held to them)."""
    im = pc.images()
    for name in ("noise_200", "zeros_256", "full_256", *pc.LEVEL6_FACTOR):
        u8 = im[name]
        raw = len(pc.filtered_stream(u8))
        for png in (encode(u8, gpu), reference(name)):
            if name == "noise_200":
                assert len(png) <= raw + 5 * (-(-raw // pc.S)) + 69
            elif name in pc.LEVEL6_FACTOR:
                level6 = len(dataset_io.encode_png(u8, 6))
                print(name, len(png), "level 6", level6, "factor %.3f" % (len(png) / level6))
                assert len(png) <= pc.LEVEL6_FACTOR[name] * level6
            else:
                print(name, len(png), "of", raw)
                assert len(png) <= 0.04 * raw


def _small_generator(path, name, gpu, **kw):
    from signerf_amd.datasetgenerator import DatasetGenerator, DatasetGeneratorConfig

    size = 64
    cfg = DatasetGeneratorConfig(path=path, dataset_name=name, fx=1.2 * size, fy=1.2 * size, cx=size / 2, cy=size / 2, width=size, height=size,
                                 rows=3, cols=3, mask_dialation=(7, 7))
    return DatasetGenerator(cfg, torch.eye(4)[:3], 1.0, None, device=gpu, **kw)


@pytest.fixture(scope="module")
def scene_64(gpu):
    from helpers import make_model, small_config
    from signerf_amd import random_sphere_poses, scene

    cfg = small_config(num_proposal_samples_per_ray=(64, 32), num_nerf_samples_per_ray=24)
    model, _ = make_model(cfg, gpu, density_bias=5.0)
    ref = scene.benchmark_cameras(8)[:, :3]
    torch.manual_seed(1)
    syn = random_sphere_poses(2, torch.device("cpu"), 0.5, (30.0, 120.0), (0.0, 360.0), [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])[:, :3]
    return model, ref, syn


def test_same_bytes_twice_and_on_a_side_stream_beside_a_render(gpu, reference, scene_64, tmp_path):
    from signerf_amd import Cameras
    from signerf_amd.datasetgenerator import render_camera

    model, _, syn = scene_64
    gen = _small_generator(tmp_path, "unused", gpu)
    cams = Cameras(syn, 1.2 * 64, 1.2 * 64, 32.0, 32.0, 64, 64).to(gpu)
    for name in ("smooth_noise_200", "stream_2S+1"):
        t = torch.from_numpy(np.array(pc.images()[name])).to(gpu)
        first = dataset_io.encode_png_hip(t)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        rgb, _, _ = render_camera(gen.config, model, cams[0])      # in flight on the current stream
        with torch.cuda.stream(side):
            second = dataset_io.encode_png_hip(t)
        torch.cuda.synchronize()
        assert first == second == reference(name)
        assert bool(torch.isfinite(rgb).all())


def test_refusals_leave_the_next_encode_unchanged(gpu, reference):
    lib = _lib.load()
    u8 = pc.images()["37x53x3"]
    t = torch.from_numpy(np.array(u8)).to(gpu)
    h, w, c = u8.shape
    ws_bytes, cap = lib.sn_png_workspace_bytes(h, w, c), lib.sn_png_max_file_bytes(h, w, c)
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device=gpu)
    out = torch.empty(8 + cap, dtype=torch.uint8, device=gpu)
    big = 1 << 40

    def call(image=t.data_ptr(), h=h, w=w, c=c, ws_ptr=ws.data_ptr(), ws_bytes=ws_bytes, file=out.data_ptr() + 8, cap=cap, count=out.data_ptr()):
        return lib.sn_png_encode(image, h, w, c, ws_ptr, ws_bytes, file, cap, count, _lib.current_stream())

    def good():
        out.zero_()
        assert call() == 0
        torch.cuda.synchronize()
        host = out.cpu()
        return host[8:8 + int(host[:8].view(torch.int64).item())].numpy().tobytes()

    before = good()
    assert before == reference("37x53x3")
    refusals = [dict(image=None), dict(ws_ptr=None), dict(file=None), dict(count=None), dict(c=0, ws_bytes=big, cap=big), dict(c=2, ws_bytes=big, cap=big),
                dict(c=4, ws_bytes=big, cap=big), dict(h=0, ws_bytes=big, cap=big), dict(h=8193, ws_bytes=big, cap=big), dict(w=0, ws_bytes=big, cap=big),
                dict(w=8193, ws_bytes=big, cap=big), dict(ws_bytes=ws_bytes - 1), dict(cap=cap - 1), dict(ws_ptr=ws.data_ptr() + 4)]
    for kw in refusals:
        assert call(**kw) == _lib.SN_ERR_INVALID, kw
        assert b"sn_png_encode" in lib.sn_last_error(None), kw
        assert good() == before, kw


def test_generated_dataset_hip_against_native(gpu, tmp_path):
    from PIL import Image

    g = torch.Generator().manual_seed(3)
    rgb, mask = torch.rand(20, 24, 3, generator=g).to(gpu), (torch.rand(20, 24, 1, generator=g) > 0.5).float().to(gpu)
    files = {}
    for enc, workers in (("native", 0), ("hip", 0), ("hip", 2)):
        ds = dataset_io.GeneratedDataset(tmp_path, f"{enc}{workers}", png_encoder=enc, save_workers=workers)
        ds.init_directory()
        ds.save_image(rgb, ds.dirs["images"] / "image_0.png")
        ds.save_image(mask, ds.dirs["masks"] / "mask_0.png")
        ds.close()
        files[(enc, workers)] = [(ds.dirs["images"] / "image_0.png").read_bytes(), (ds.dirs["masks"] / "mask_0.png").read_bytes()]
    assert files[("hip", 0)] == files[("hip", 2)] and files[("hip", 0)] != files[("native", 0)]
    for k in range(2):
        a, b = Image.open(io.BytesIO(files[("native", 0)][k])), Image.open(io.BytesIO(files[("hip", 0)][k]))
        assert a.mode == b.mode == ("RGB", "L")[k] and np.array_equal(np.asarray(a), np.asarray(b))
    want = dataset_io.tensor_to_uint8(rgb).cpu().numpy()
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[("hip", 0)][0]))), want)


def test_dataset_generator_hip_against_native(gpu, scene_64, tmp_path):
    from PIL import Image

    model, ref, syn = scene_64
    for enc in ("native", "hip"):
        _small_generator(tmp_path, enc, gpu, png_encoder=enc).generate_dataset(model, ref, synthetic_camera_to_worlds=syn)
    a, b = tmp_path / "native", tmp_path / "hip"
    assert json.load(open(a / "transforms.json")) == json.load(open(b / "transforms.json"))
    assert (a / "transforms.json").read_bytes() == (b / "transforms.json").read_bytes()
    pngs = sorted(os.path.relpath(os.path.join(d, f), a) for d, _, fs in os.walk(a) for f in fs if f.endswith(".png"))
    assert pngs == sorted(os.path.relpath(os.path.join(d, f), b) for d, _, fs in os.walk(b) for f in fs if f.endswith(".png"))
    assert len(pngs) >= 8 * (8 + 2)
    hip_written = 0
    for rel in pngs:
        x, y = Image.open(a / rel), Image.open(b / rel)
        assert x.mode == y.mode and np.array_equal(np.asarray(x), np.asarray(y)), rel
        hip_written += (b / rel).read_bytes()[41:43] == b"\x78\x01" and (a / rel).read_bytes() != (b / rel).read_bytes()
    assert hip_written >= 8 * (8 + 2)      # the views' files really came from the GPU encoder
