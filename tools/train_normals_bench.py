#!/usr/bin/env python3
"""Which route to the analytic normals of training samples is faster (signerf_amd/train_normals.py): the fused kernel of
csrc/sn_train_normals.h, or the composed route -- the hash encoding, ``sn_mlp_backward`` of the one-hot gradient and
``sn_hashgrid_backward`` for ``grad_q``, then ``F.normalize`` --, and what ``training_normals`` adds to a training step.  The result decides
which of the two ``NerfactoField.forward_training`` calls (DESIGN.md §4 "Training-mode normals", "Measurement"); recorded, not gated.

Shape: 4096 rays x 48 samples, ray-ordered (consecutive samples of a ray, contracted as the field contracts them), the default field:
L = 16, F = 2, T = 2^19, the stack 32 -> 64 -> 16.  Same process, the two routes ALTERNATING rep by rep, every rep one hipEvent span
that ends in a synchronise, after a warm-up of both; the outputs of the two routes are compared on the same inputs.  Then the whole
training step of a ``predict_normals`` nerfacto (4096 rays, ``get_training_outputs`` -> ``get_loss_dict`` -> ``backward()``) with
``training_normals`` off, on through the fused kernel and on through the composed route, alternating the same way.

    python tools/train_normals_bench.py [--reps 40] [--out profiles/train_normals_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from signerf_amd import train_normals  # noqa: E402
from signerf_amd.cameras import RayBundle  # noqa: E402
from signerf_amd.config import NerfactoModelConfig  # noqa: E402
from signerf_amd.nerfacto import MLPWithHashEncoding  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=4096)
ap.add_argument("--samples", type=int, default=48)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_normals_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda", 0)


def alternate(fns):
    """{name: fn} -> {name: {ms_median, ms_min, ms_p90}}: every rep runs each fn once, in turn, one event span each."""
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_p90": round(sorted(t)[int(0.9 * (len(t) - 1))], 4)}
            for k, t in times.items()}


# ---- the two routes on the field's own shape -------------------------------------------------------------------------------------------------
R, S = a.rays, a.samples
gen = torch.Generator().manual_seed(0)
o = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * 0.5
d = torch.nn.functional.normalize(torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * 0.2 - o, dim=-1)
t = torch.sort(torch.rand(R, S, generator=gen) * 3.95 + 0.05, dim=-1).values
pos = o[:, None, :] + d[:, None, :] * t[..., None]
mag = torch.linalg.norm(pos, ord=float("inf"), dim=-1)[..., None]
q = ((torch.where(mag < 1, pos, (2 - (1 / mag)) * (pos / mag)) + 2.0) / 4.0).reshape(-1, 3).contiguous().to(dev)
torch.manual_seed(0)
base = MLPWithHashEncoding(16, 16, 2048, 19, 2, 2, 64, 16).to(dev)
table, scalings = base.encoder.hash_table.detach(), base.encoder.scalings().to(dev)
weights, biases = [layer.weight.detach() for layer in base.mlp.layers], [layer.bias.detach() for layer in base.mlp.layers]
args = (q, table, scalings, 19, weights, biases)

fused, fused_g = train_normals.analytic_normals(*args, return_grad=True)
composed, composed_g = train_normals.analytic_normals_composed(*args, return_grad=True)
agree = {"grad_q_max_abs_difference": float((fused_g - composed_g).abs().max()), "grad_q_max_abs": float(composed_g.abs().max()),
         "normals_max_abs_difference": float((fused - composed).abs().max())}
print("agreement", json.dumps(agree), flush=True)
routes = alternate({"fused": lambda: train_normals.analytic_normals(*args), "composed": lambda: train_normals.analytic_normals_composed(*args)})
routes["composed_over_fused"] = round(routes["composed"]["ms_median"] / routes["fused"]["ms_median"], 3)
routes["points"] = R * S
print("routes", json.dumps(routes), flush=True)
del base, fused, composed, fused_g, composed_g
torch.cuda.empty_cache()

# ---- the whole training step ------------------------------------------------------------------------------------------------------------------
step_rec = {}
if not a.no_step:
    bundle = RayBundle(origins=o.to(dev), directions=d.to(dev), pixel_area=torch.ones(R, 1, device=dev),
                       camera_indices=torch.randint(0, 4, (R, 1), generator=gen).to(dev))
    batch = {"image": torch.rand(R, 3, generator=gen).to(dev)}
    for impl in ("hip", "torch"):
        models = {}
        for name, on in (("off", False), ("on_fused", True), ("on_composed", True)):
            torch.manual_seed(0)
            models[name] = NerfactoModelConfig(training_forward=True, training_mlp=impl, num_train_data=4, camera_optimizer_mode="off", predict_normals=True,
                                               training_normals=on).setup().to(dev)
            models[name].train()
        field = models["on_composed"].field       # this one model's field takes the composed route
        field._training_analytic_normals = lambda q, f=field: train_normals.analytic_normals_composed(
            q, f.mlp_base.encoder.hash_table, f.mlp_base.encoder._scalings_on(q.device), f.mlp_base.encoder.log2_hashmap_size,
            [layer.weight for layer in f.mlp_base.mlp.layers], [layer.bias for layer in f.mlp_base.mlp.layers])
        at = {k: 0 for k in models}

        def train_step(name):
            model = models[name]
            model.zero_grad(set_to_none=True)
            model.set_training_step(at[name])
            at[name] += 1
            out = model(bundle)
            sum(model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch)).values()).backward()

        rec = alternate({name: (lambda name=name: train_step(name)) for name in models})
        rec["on_fused_minus_off_ms"] = round(rec["on_fused"]["ms_median"] - rec["off"]["ms_median"], 4)
        rec["on_composed_minus_off_ms"] = round(rec["on_composed"]["ms_median"] - rec["off"]["ms_median"], 4)
        step_rec["training_mlp=" + impl] = rec
        print("training_step", impl, json.dumps(rec), flush=True)
        del models
        torch.cuda.empty_cache()

doc = {"tool": "tools/train_normals_bench.py", "device": torch.cuda.get_device_name(0), "rays": R, "samples": S, "reps": a.reps, "warmup": a.warmup,
       "note": "ms per call, hipEvent spans ending in a synchronise, the variants alternating rep by rep in one process.  `routes`: the analytic "
               "normals of rays x samples ray-ordered points on the default field (L 16, F 2, T 2^19, 32 -> 64 -> 16), fused kernel against the "
               "composed route (hash encoding + sn_mlp_backward + sn_hashgrid_backward + F.normalize).  `training_step`: a predict_normals nerfacto, "
               "levels (256, 96, 48), forward + losses + backward, no optimiser; training_normals off, on with the field on the fused kernel, on with "
               "the field on the composed route",
       "agreement": agree, "routes": routes, "training_step": step_rec}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", a.out)
