#!/usr/bin/env python3
"""png_encoder="hip" against the host encoders (DESIGN.md §4 "PNG encoding"): writes profiles/png_hip_bench.json.

  * encode time and file size of one 800x800x3 render and its 800x800x1 mask, taken from the trained scene's outputs
    (tools/make_trained_scene.py): ``encode_png_hip`` (device-synchronised: its one wait is inside), ``encode_png`` at zlib levels 6 and 1
    on 1 thread and on the granted threads; >= 50 interleaved repetitions, medians; ms per image and MB/s of pixels; and the hip leg
    split by device events into its kernels and its copy-back.
  * the generator loop tools/config5_bench.py times (8 + 50 views, 800x800) with "native" at level 6, "native" at level 1, "hip", and PNG
    writes off, interleaved, medians.

    python tools/png_bench.py [--reps 50] [--loop-reps 3] [--legs native6,native1,hip,off] [--out profiles/png_hip_bench.json]

A tree without the "hip" encoder (the parent commit) runs the other legs into a file of its own (profiles/png_parent_bench.json):
--legs native6,native1,off --no-hip --out profiles/png_parent_bench.json."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from signerf_amd import Cameras, _lib, dataset_io, random_sphere_poses, scene  # noqa: E402
from signerf_amd.datasetgenerator import DatasetGenerator, DatasetGeneratorConfig, render_camera  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--views", type=int, default=50)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--loop-reps", type=int, default=3)
ap.add_argument("--threads", type=int, default=16, help="the granted host threads")
ap.add_argument("--legs", default="native6,native1,hip,off")
ap.add_argument("--no-hip", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_hip_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
S = a.size

import make_trained_scene as mts  # noqa: E402

cfg = scene.proposal_config()
model = cfg.setup()
sd, _ = mts.trained_state_dict(cfg, device="cuda")
model.load_state_dict(sd, strict=False)
model.field.embedding_appearance.embedding.weight.data.copy_(sd["field.embedding_appearance.embedding.weight"])
model = model.to(dev).eval()
ref = scene.benchmark_cameras(8)[:, :3]
torch.manual_seed(1)
syn = random_sphere_poses(a.views, torch.device("cpu"), 0.5, (30.0, 120.0), (0.0, 360.0), [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])[:, :3]
tmp = tempfile.mkdtemp(prefix="signerf_png_bench_")


def generator_config(name):
    return DatasetGeneratorConfig(path=tmp, dataset_name=name, fx=1.2 * S, fy=1.2 * S, cx=S / 2, cy=S / 2, width=S, height=S, rows=3, cols=3)


out = {"size": [S, S], "views": 8 + a.views, "threads": a.threads, "scene": "trained (tools/make_trained_scene.py)", "reps": a.reps}

# ---- one render and its mask -------------------------------------------------------------------------------------------------------------
cams = Cameras(syn, 1.2 * S, 1.2 * S, S / 2, S / 2, S, S).to(dev)
rgb, mask, _ = render_camera(generator_config("x"), model, cams[0])
images = {"render_800x800x3": dataset_io.tensor_to_uint8(rgb), "mask_800x800x1": dataset_io.tensor_to_uint8(mask.float())}
torch.cuda.synchronize()
pool = ThreadPoolExecutor(max_workers=a.threads)
enc = {}
for name, u8 in images.items():
    host = u8.cpu().numpy()
    legs = {}
    if not a.no_hip:
        legs["hip"] = lambda: dataset_io.encode_png_hip(u8)
    for level in (6, 1):
        legs[f"native_level_{level}_1_thread"] = lambda level=level: dataset_io.encode_png(host, level)
        # the granted threads each encode one image: time per image = wall / threads
        legs[f"native_level_{level}_{a.threads}_threads"] = lambda level=level: list(pool.map(lambda _: dataset_io.encode_png(host, level), range(a.threads)))
    times, sizes = {k: [] for k in legs}, {}
    for rep in range(a.reps + 2):
        for k, f in legs.items():   # interleaved
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            if rep >= 2:
                times[k].append(dt / (a.threads if k.endswith("_threads") else 1))
            sizes[k.replace(f"_{a.threads}_threads", "").replace("_1_thread", "")] = len(r[0] if isinstance(r, list) else r)
    enc[name] = {"pixel_bytes": host.size, "file_bytes": sizes,
                 "ms_per_image": {k: statistics.median(v) * 1e3 for k, v in times.items()},
                 "pixel_MB_per_s": {k: host.size / statistics.median(v) / 1e6 for k, v in times.items()}}
    if not a.no_hip:   # the hip leg split by device events: the three kernels, then the one copy of the file buffer to pinned memory
        lib, slot = _lib.load(), dataset_io._PngHipSlot(*u8.shape, dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        kernels, copy = [], []
        for rep in range(a.reps + 2):
            base = slot.out.data_ptr()
            ev[0].record()
            _lib.check(lib.sn_png_encode(u8.data_ptr(), *u8.shape, slot.workspace.data_ptr(), slot.workspace.numel(), base + 8, slot.capacity, base,
                                         _lib.current_stream()), None, "sn_png_encode")
            ev[1].record()
            slot.host.copy_(slot.out, non_blocking=True)
            ev[2].record()
            ev[2].synchronize()
            if rep >= 2:
                kernels.append(ev[0].elapsed_time(ev[1]))
                copy.append(ev[1].elapsed_time(ev[2]))
        enc[name]["hip_split_ms"] = {"kernels": statistics.median(kernels), "copy_back": statistics.median(copy), "copied_bytes": 8 + slot.capacity}
pool.shutdown()
out["encode"] = enc

# ---- the generator loop ------------------------------------------------------------------------------------------------------------------
LEGS = {"native6": dict(write_images=True, png_compress_level=None, png_encoder="native"), "native1": dict(write_images=True, png_compress_level=1, png_encoder="native"),
        "hip": dict(write_images=True, png_compress_level=None, png_encoder="hip"), "off": dict(write_images=False)}
legs = [l for l in a.legs.split(",") if l and not (a.no_hip and l == "hip")]
loop = {l: [] for l in legs}
for rep in range(a.loop_reps + 1):   # the first repetition warms the handle, the streams and the allocator
    for l in legs:
        gen = DatasetGenerator(generator_config(f"{l}{rep}"), torch.eye(4)[:3], 1.0, None, device=dev, save_workers=None, profile=True, **LEGS[l])
        torch.cuda.synchronize()
        t = time.perf_counter()
        gen.generate_dataset(model, ref, synthetic_camera_to_worlds=syn)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        if rep > 0:
            loop[l].append({"total_ms": dt * 1e3, "save_ms": gen.timings.get("save_s", 0) * 1e3})
        shutil.rmtree(os.path.join(tmp, f"{l}{rep}"), ignore_errors=True)
    print(rep, {l: (loop[l][-1]["total_ms"] if loop[l] else None) for l in legs}, flush=True)
out["generator_loop"] = {l: {"median_total_ms": statistics.median(x["total_ms"] for x in v), "median_save_ms": statistics.median(x["save_ms"] for x in v),
                             "all_total_ms": [x["total_ms"] for x in v]} for l, v in loop.items()}
shutil.rmtree(tmp, ignore_errors=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
