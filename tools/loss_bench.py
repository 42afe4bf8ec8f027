#!/usr/bin/env python3
"""What the back half of a training step costs (signerf_amd/losses.py over csrc/sn_losses.h) beside the same formulas as plain torch ops on
the same GPU.  Recorded, not gated (DESIGN.md §4 "Training back half").

Shapes: SIGNeRF's ``train_num_rays_per_batch`` R = 16384 with nerfacto's levels (256, 96, 48): compositing of the 48 main samples, the
distortion loss of the main level (torch: an [R, 48, 48] pairwise tensor), the interlevel loss of the two proposal levels against it.
Every figure is forward + backward, the median of 50 hipEvent spans after a warm-up.

    python tools/loss_bench.py [--reps 50] [--out profiles/loss_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import loss_oracle as lo  # noqa: E402
from signerf_amd import losses  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=16384)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
R, LEVELS = a.rays, (256, 96, 48)
S = LEVELS[-1]

deltas, density, colour = (x.to(dev) for x in lo.composite_inputs(R, S, seed=0))
hist = [tuple(x.to(dev) for x in lo.histogram_inputs(R, n, seed=1 + i)) for i, n in enumerate(LEVELS)]
t_main, w_main = hist[-1]


def span(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"ms_median": round(statistics.median(times), 4), "ms_min": round(min(times), 4)}


def composite_step(hip):
    dn, c = density.clone().requires_grad_(), colour.clone().requires_grad_()

    def fn():
        dn.grad = c.grad = None
        if hip:
            w, rgb, acc = losses.composite(dn[..., None], c, deltas[..., None])
        else:
            w, rgb, acc = lo.composite(deltas, dn, c)
        (rgb.sum() + acc.sum() + w.sum()).backward()
    return fn


def distortion_step(hip):
    w = w_main.clone().requires_grad_()

    def fn():
        w.grad = None
        (losses.lossfun_distortion(t_main, w) if hip else lo.lossfun_distortion(t_main, w)).mean().backward()
    return fn


def interlevel_step(hip):
    envs = [(t, w.clone().requires_grad_()) for t, w in hist[:-1]]

    def fn():
        total = 0.0
        for t_env, w_env in envs:
            w_env.grad = None
            f = losses.lossfun_outer if hip else lo.lossfun_outer
            total = total + f(t_main, w_main, t_env, w_env).mean()
        total.backward()
    return fn


results = {}
for name, step in (("composite", composite_step), ("distortion", distortion_step), ("interlevel", interlevel_step)):
    rec = {"hip": span(step(True)), "torch": span(step(False))}
    rec["torch_over_hip"] = round(rec["torch"]["ms_median"] / rec["hip"]["ms_median"], 2)
    results[name] = rec
    print(name, json.dumps(rec), flush=True)
doc = {"tool": "tools/loss_bench.py", "device": torch.cuda.get_device_name(0), "rays": R, "levels": list(LEVELS), "reps": a.reps,
       "note": "forward + backward per call, ms, median of hipEvent spans; `torch`: tests/loss_oracle.py's plain torch ops in fp32 on the same GPU",
       "results": results}
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", a.out)
