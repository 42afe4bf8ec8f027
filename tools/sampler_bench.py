#!/usr/bin/env python3
"""What training-mode proposal sampling costs (signerf_amd/samplers.py over csrc/sn_sampler.h) beside the same three steps as plain torch
ops (tests/sampler_oracle.py in fp32) on the same GPU, in the same process.  Recorded, not gated (DESIGN.md §4 "Training-mode sampling").

Shapes: the three sampler launches of a nerfacto step at 4096 rays -- the initial sampler (256 samples) and the two resampling steps
(256 -> 96, 96 -> 48) --, single jitter, piecewise spacing, the collider's planes; every output a ``RaySamples`` carries is produced on both
sides (spacing and Euclidean bins, deltas, positions, q, selector), the random numbers included (Philox in the kernels, ``torch.rand`` in
the torch ops).  The weights a resampling step reads are rand^8 rows, as in the tests.  Per launch and for the three together: the
median of 50 hipEvent spans after a warm-up.

    python tools/sampler_bench.py [--reps 50] [--out profiles/sampler_bench.json]
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

import sampler_oracle as so  # noqa: E402
from signerf_amd import RayBundle, samplers  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=4096)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
LEVELS = (256, 96, 48)
NEAR, FAR, ANNEAL = 0.05, 1000.0, 0.35


def span(fn):
    for _ in range(a.warmup):
        fn()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4)}


R = a.rays
o, d, _, _ = so.rays(R, seed=0)
o, d = o.to(dev), d.to(dev)
bundle = RayBundle(origins=o, directions=d, pixel_area=torch.ones(R, 1, device=dev), camera_indices=torch.zeros(R, 1, dtype=torch.long, device=dev))
nears, fars = torch.full((R,), NEAR, device=dev), torch.full((R,), FAR, device=dev)
weights = [so.weights(R, n, seed=n).to(dev) for n in LEVELS[:2]]
base = torch.linspace(0.0, 1.0, LEVELS[0] + 1).to(dev)
grids = [so.u_grid(m).to(dev) for m in LEVELS[1:]]
common = dict(near_plane=NEAR, far_plane=FAR, single_jitter=True, seed=1)

# the inputs of the resampling steps: the previous level as the kernels produce it
level0 = samplers.sample_initial(bundle, LEVELS[0], offset=0, **common)
level1 = samplers.sample_pdf(bundle, level0, weights[0][..., None], LEVELS[1], anneal=ANNEAL, offset=1, **common)


def hip_initial():
    return samplers.sample_initial(bundle, LEVELS[0], offset=0, **common)


def hip_pdf(k):
    prev = (level0, level1)[k]
    return samplers.sample_pdf(bundle, prev, weights[k][..., None], LEVELS[k + 1], anneal=ANNEAL, offset=k + 1, **common)


def torch_tail(sbins):
    eb = so.euclid(sbins, nears, fars, "piecewise")
    return (sbins, eb) + so.samples(eb, o, d)


def torch_initial():
    return torch_tail(so.initial_bins(base, torch.rand(R, device=dev)))


def torch_pdf(k):
    prev = (level0, level1)[k].spacing_bins
    u = so.train_u(grids[k], torch.rand(R, device=dev))
    return torch_tail(so.pdf_bins(prev, weights[k], u, anneal=ANNEAL)[0])


results = {}
for name, hip, ref in (("initial_256", hip_initial, torch_initial), ("pdf_256_to_96", lambda: hip_pdf(0), lambda: torch_pdf(0)),
                       ("pdf_96_to_48", lambda: hip_pdf(1), lambda: torch_pdf(1)),
                       ("step_three_launches", lambda: (hip_initial(), hip_pdf(0), hip_pdf(1)), lambda: (torch_initial(), torch_pdf(0), torch_pdf(1)))):
    results[name] = {"hip": span(hip), "torch": span(ref)}
    results[name]["torch_over_hip"] = round(results[name]["torch"]["ms_median"] / results[name]["hip"]["ms_median"], 2)
    print(name, results[name], flush=True)

out = {"tool": "tools/sampler_bench.py", "device": torch.cuda.get_device_name(0), "rays": R, "levels": list(LEVELS), "reps": a.reps,
       "note": "ms per call, median of hipEvent spans; `hip`: signerf_amd.samplers (one launch per level, output allocation and the RaySamples "
               "views included); `torch`: tests/sampler_oracle.py as fp32 torch ops on the same GPU in the same process, torch.rand included",
       "results": results}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(a.out)
