#!/usr/bin/env python3
"""What the trainable MLP costs (signerf_amd/mlp.py over csrc/sn_mlp.h) beside the same ``nn.Linear`` stack as torch ops with autograd
(``MLP.forward`` with implementation="torch") on the same GPU, in the same process.  Recorded, not gated (DESIGN.md §4 "Trainable MLP").

Stacks at the sizes of a nerfacto step at 4096 rays with (256, 96, 48) samples per ray: the main field's base (32, 64, 16) and head
(63, 64, 64, 3) on 196 608 points, the proposal nets' (10, 16, 1) on 1 048 576 and 393 216 points.  Per stack, forward + backward (input
and parameter gradients), the median of 50 hipEvent spans after a warm-up.  Then one whole training step of the default model (4096 rays,
``get_training_outputs`` -> ``get_loss_dict`` -> ``backward()``) with ``training_mlp`` set each way.

``--precision fp16`` measures the mixed-precision arithmetic instead (DESIGN.md §4 "Mixed-precision MLP"): the same four stacks and the same
whole step on the HIP MLP with ``precision`` "fp32" and "fp16", in the same process -- the base of every fp16 figure is the fp32 figure of
the same run -- written to profiles/mlp_bench_half.json.

    python tools/mlp_bench.py [--reps 50] [--out profiles/mlp_bench.json]
    python tools/mlp_bench.py --precision fp16 [--out profiles/mlp_bench_half.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from signerf_amd.cameras import RayBundle  # noqa: E402
from signerf_amd.config import NerfactoModelConfig  # noqa: E402
from signerf_amd.nerfacto import MLP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=4096)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--precision", choices=("fp32", "fp16"), default="fp32", help="fp16: time the HIP MLP in fp32 and in fp16 instead of hip against torch")
ap.add_argument("--out", default=None, help="default: profiles/mlp_bench.json, or profiles/mlp_bench_half.json with --precision fp16")
a = ap.parse_args()
HALF = a.precision == "fp16"
a.out = a.out or os.path.join(ROOT, "profiles", "mlp_bench_half.json" if HALF else "mlp_bench.json")
# (label, MLP.implementation / training_mlp, MLP.precision / training_mlp_precision) of the two sides; the ratio is second over first
SIDES = [("fp16", "hip", "fp16"), ("fp32", "hip", "fp32")] if HALF else [("hip", "hip", "fp32"), ("torch", "torch", "fp32")]
RATIO = SIDES[1][0] + "_over_" + SIDES[0][0]
dev = torch.device("cuda", 0)
STACKS = {"main_base": (48, (32, 64, 16)), "main_head": (48, (63, 64, 64, 3)), "proposal_0": (256, (10, 16, 1)), "proposal_1": (96, (10, 16, 1))}


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


results = {}
for name, (samples, dims) in STACKS.items():
    N = a.rays * samples
    torch.manual_seed(len(name))
    net = MLP(dims[0], len(dims) - 1, dims[1], dims[-1]).to(dev)
    gen = torch.Generator().manual_seed(1)
    x = (torch.rand(N, dims[0], generator=gen) * 2 - 1).to(dev).requires_grad_()
    g = torch.randn(N, dims[-1], generator=gen).to(dev)

    def step():
        x.grad = None
        net.zero_grad(set_to_none=True)
        net(x).backward(g)

    def forward():
        with torch.no_grad():
            net(x)

    rec = {"points": N, "dims": list(dims)}
    for label, impl, precision in SIDES:
        net.implementation, net.precision = impl, precision
        rec[label] = span(step)
        rec[label + "_forward"] = span(forward)
    rec[RATIO] = round(rec[SIDES[1][0]]["ms_median"] / rec[SIDES[0][0]]["ms_median"], 2)
    results[name] = rec
    print(name, json.dumps(rec), flush=True)
    del net, x, g
    torch.cuda.empty_cache()

step_rec = {}
if not a.no_step:
    R = a.rays
    gen = torch.Generator().manual_seed(0)
    o = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * 0.5
    look = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * 0.2
    bundle = RayBundle(origins=o.to(dev), directions=torch.nn.functional.normalize(look - o, dim=-1).to(dev), pixel_area=torch.ones(R, 1, device=dev),
                       camera_indices=torch.randint(0, 4, (R, 1), generator=gen).to(dev))
    batch = {"image": torch.rand(R, 3, generator=gen).to(dev)}
    for label, impl, precision in SIDES:
        torch.manual_seed(0)
        model = NerfactoModelConfig(training_forward=True, training_mlp=impl, training_mlp_precision=precision, num_train_data=4,
                                    camera_optimizer_mode="off").setup().to(dev)
        model.train()
        at = [0]

        def train_step():
            model.zero_grad(set_to_none=True)
            model.set_training_step(at[0])
            at[0] += 1
            out = model(bundle)
            sum(model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch)).values()).backward()

        step_rec[label] = span(train_step)
        print("training_step", label, json.dumps(step_rec[label]), flush=True)
        del model
        torch.cuda.empty_cache()
    step_rec[RATIO] = round(step_rec[SIDES[1][0]]["ms_median"] / step_rec[SIDES[0][0]]["ms_median"], 2)

other = ("`fp32` / `fp16`: the MLP module on implementation=\"hip\" with that precision, same GPU, same process" if HALF else
         "`torch`: the same MLP module on implementation=\"torch\" (nn.Linear + relu with autograd) on the same GPU in the same process")
doc = {"tool": "tools/mlp_bench.py" + (" --precision fp16" if HALF else ""), "device": torch.cuda.get_device_name(0), "rays": a.rays, "reps": a.reps,
       "note": "forward + backward (input and parameter gradients) per call, ms, median of hipEvent spans; " + other + "; `training_step`: the "
               "default nerfacto, 4096 rays, levels (256, 96, 48), forward + losses + backward, no optimiser",
       "results": results, "training_step": step_rec}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", a.out)
