#!/usr/bin/env python3
"""What a wide field (hidden_dim = hidden_dim_color = 128, nerfacto-big; csrc/sn_wide_kernels.h) costs per frame, beside the default-width
field in exact fp32 from the same call.  Recorded, not gated (DESIGN.md §4 "Wide fields"):

  * 800x800x64 uniform sampler (BASELINE.json configs[1]'s shape) at log2_hashmap_size 19 and 21,
  * 800x800 behind the proposal sampler with (256, 128) proposal samples + 128 main samples.

Warm-up, then >= 100 timed frames per field, interleaved wide / default, every frame device-synchronised (one launch at a time).

    python tools/wide_bench.py [--frames 100] [--out profiles/wide_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from helpers import make_model  # noqa: E402
from signerf_amd import Cameras, scene  # noqa: E402
from signerf_amd.config import SIGNeRFModelConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_bench.json"))
a = ap.parse_args()
assert a.frames >= 100, "at least 100 timed frames"
dev = torch.device("cuda", 0)
warnings.simplefilter("ignore", RuntimeWarning)
W = H = 800
bundle = Cameras(scene.benchmark_cameras(8)[:, :3], 800.0, 800.0, W / 2, H / 2, W, H).to(dev)[0].generate_rays(0)


def models(**kw):
    out = {}
    for name, width in (("wide", 128), ("default", 64)):
        cfg = SIGNeRFModelConfig(hidden_dim=width, hidden_dim_color=width, precision="fp32", predict_normals=False, **kw)
        out[name] = make_model(cfg, dev, head_gain=6.0 if width == 128 else 3.0)[0].eval()
    return out


def run(tag, samples_per_ray, **kw):
    ms = models(**kw)
    times = {k: [] for k in ms}
    for m in ms.values():
        for _ in range(a.warmup):
            m.get_outputs_for_camera_ray_bundle(bundle)
    torch.cuda.synchronize()
    for _ in range(a.frames):
        for k, m in ms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m.get_outputs_for_camera_ray_bundle(bundle)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    rec = {"config": tag, "width": W, "height": H, "field_samples_per_ray": samples_per_ray, "frames": a.frames}
    for k, t in times.items():
        med = statistics.median(t)
        rec[k] = {"precision": "fp32 (exact fp32 MFMA)", "ms_per_frame_median": round(med, 4), "ms_per_frame_min": round(min(t), 4),
                  "ray_samples_per_s": round(W * H * samples_per_ray / (med * 1e-3), 1)}
    rec["wide_over_default"] = round(rec["wide"]["ms_per_frame_median"] / rec["default"]["ms_per_frame_median"], 3)
    print(json.dumps(rec), flush=True)
    del ms
    torch.cuda.empty_cache()
    return rec


results = [
    run("800x800x64 uniform sampler, T = 2^19", 64, num_proposal_iterations=0, num_nerf_samples_per_ray=64, log2_hashmap_size=19),
    run("800x800x64 uniform sampler, T = 2^21, max_res 4096", 64, num_proposal_iterations=0, num_nerf_samples_per_ray=64, log2_hashmap_size=21, max_res=4096),
    run("800x800 proposal sampler (256, 128) + 128, T = 2^19", 128, num_proposal_iterations=2, num_proposal_samples_per_ray=(256, 128),
        num_nerf_samples_per_ray=128, log2_hashmap_size=19),
]
doc = {"tool": "tools/wide_bench.py", "device": torch.cuda.get_device_name(0),
       "note": "ms per render call (all kernels of the frame), median of interleaved device-synchronised frames; ray_samples_per_s counts main-field samples",
       "mfma_prediction": "a wide field issues 28 672 multiply-adds per sample on the matrix cores against 10 240: about 2.8x the default-width exact-fp32 time",
       "results": results}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", a.out)
