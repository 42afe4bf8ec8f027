#!/usr/bin/env python3
"""Ray batches across cameras: one launch of sn_generate_ray_batch against the only route there was before it, a Python loop over the
cameras present in the batch calling ``cams[b].generate_rays(0, coords=coords[c == b])`` with boolean masks.

The set: 58 cameras at 800 x 800 (the 58-view set of BASELINE configs[4]: circle_poses(58), radius 0.5) with a uint8 image stack.
Batches: N = 4096 in random order (nerfacto's train_num_rays_per_batch), N = 4096 in 32 x 32-patch order (PatchPixelSampler), N = 2^20 in
both orders; each with and without the pixel gather.  The loop is timed in the same run on the N = 4096 batches (and once, with fewer
repetitions, at 2^20).  Times are hipEvent intervals on the stream, medians of --reps after --warmup; the loop's span includes its host
work (58 launches and 58 boolean-mask selections, each a device -> host sync), which is what a caller of it waits for.

    python tools/ray_batch_bench.py [--reps 50] [--json profiles/ray_batch_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from signerf_amd import Cameras, PatchPixelSamplerConfig, PixelSamplerConfig, scene  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) for a, b in ev]
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def loop_over_cameras(cams, tri, coords):
    """The parent commit's route: per camera present in the batch, a boolean mask and one launch."""
    out = torch.empty((tri.shape[0], 3), device=tri.device)
    for b in torch.unique(tri[:, 0]).tolist():
        sel = tri[:, 0] == b
        out[sel] = cams[b].generate_rays(0, coords=coords[sel]).directions
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=58)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "ray_batch_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ray_batch_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    B, S = a.cameras, a.size
    cams = Cameras(scene.benchmark_cameras(B)[:, :3], 1.2 * S, 1.2 * S, S / 2, S / 2, S, S).to(dev)
    images = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for n in (4096, 1 << 20):
        batches = {"random": PixelSamplerConfig().setup(num_rays_per_batch=n, generator=gen),
                   "patch32": PatchPixelSamplerConfig().setup(patch_size=32, num_rays_per_batch=n, generator=gen)}
        for order, sampler in batches.items():
            tri = sampler.sample_method(sampler.num_rays_per_batch, B, S, S, device=dev)
            coords = tri[:, 1:].float() + 0.5
            row = {"n": int(tri.shape[0]), "order": order, "cameras_in_batch": int(torch.unique(tri[:, 0]).numel())}
            row["batch_ms"], row["batch_min_ms"], row["batch_max_ms"] = timed(lambda: cams.generate_rays_from_indices(tri), a.reps, a.warmup)
            row["batch_pixels_ms"], _, _ = timed(lambda: cams.generate_rays_from_indices(tri, images=images), a.reps, a.warmup)
            row["batch_coords_form_ms"], _, _ = timed(lambda: cams.generate_rays(camera_indices=tri[:, 0], coords=coords), a.reps, a.warmup)
            loop_reps = a.reps if n <= 4096 else max(3, a.reps // 10)
            row["loop_ms"], row["loop_min_ms"], row["loop_max_ms"] = timed(lambda: loop_over_cameras(cams, tri, coords), loop_reps, 2)
            row["loop_over_batch"] = row["loop_ms"] / row["batch_ms"]
            same = torch.equal(loop_over_cameras(cams, tri, coords), cams.generate_rays_from_indices(tri)[0].directions)
            row["bit_identical_to_loop"] = bool(same)
            # bytes the launch must move: the triplets in, 9 floats of rays out (+ the pixels: 3 bytes in, 12 out)
            row["batch_gbytes_per_s"] = tri.shape[0] * (24 + 36) / row["batch_ms"] / 1e6
            rows.append({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()})
            print(json.dumps(rows[-1]), flush=True)
    big = {r["order"]: r for r in rows if r["n"] > 4096}
    out = {"cameras": B, "size": S, "reps": a.reps, "gpu": torch.cuda.get_device_name(0), "rows": rows,
           "random_over_patch_at_2^20": round(big["random"]["batch_ms"] / big["patch32"]["batch_ms"], 4),
           "random_over_patch_at_2^20_with_pixels": round(big["random"]["batch_pixels_ms"] / big["patch32"]["batch_pixels_ms"], 4)}
    print(json.dumps({k: v for k, v in out.items() if k != "rows"}))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
