"""The optimiser step on the default nerfacto parameter set (about 19.4 M parameters): HipAdam (signerf_amd/optimizers.py, one fused HIP
pass) against torch.optim.Adam as it comes (foreach) and with fused=True, same process, same GPU.  Four modes each: plain; under a
torch.amp.GradScaler (``scaler.step`` + ``scaler.update``); with max_norm = 1 (torch: ``clip_grad_norm_`` then ``step``); and both, which
is what a trainer iteration runs.  The gradients are put back before every span, outside it.  The median of 50 hipEvent spans after a
warm-up.  Then the whole training step of tools/mlp_bench.py (4096 rays, ``training_mlp="hip"``, forward + losses + backward) without an
optimiser and with each of the three.

    python tools/optim_bench.py [--reps 50] [--out profiles/optim_bench.json]
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
from signerf_amd.optimizers import HipAdam  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=4096)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
SCALE = 65536.0


def span(fn, before=lambda: None):
    for _ in range(a.warmup):
        before()
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"ms_median": round(statistics.median(times), 4), "ms_min": round(min(times), 4)}


def make_model():
    torch.manual_seed(0)
    model = NerfactoModelConfig(training_forward=True, training_mlp="hip", num_train_data=4, camera_optimizer_mode="off").setup().to(dev)
    model.train()
    return model, [p for p in model.parameters() if p.numel()]


BUILD = {"hip": lambda ps, max_norm=None: HipAdam(ps, lr=1e-2, eps=1e-15, max_norm=max_norm),
         "torch_foreach": lambda ps, max_norm=None: torch.optim.Adam(ps, lr=1e-2, eps=1e-15),
         "torch_fused": lambda ps, max_norm=None: torch.optim.Adam(ps, lr=1e-2, eps=1e-15, fused=True)}

model, params = make_model()
n_params = sum(p.numel() for p in params)
gen = torch.Generator().manual_seed(1)
base = [(1e-3 * torch.randn(p.shape, generator=gen)).to(dev) for p in params]
scaled = [g * SCALE for g in base]
for p in params:
    p.grad = torch.zeros_like(p)
grads = [p.grad for p in params]
results = {}
for name, build in BUILD.items():
    rec = {}
    for mode in ("plain", "scaler", "max_norm", "scaler_max_norm"):
        clip, amp = "max_norm" in mode, "scaler" in mode
        opt = build(params, 1.0 if clip else None)
        scaler = torch.amp.GradScaler("cuda", init_scale=SCALE, growth_interval=10**9, enabled=amp)
        scaler.scale(torch.zeros((), device=dev))       # (creates the scale tensor)
        outside = clip and name != "hip"                # torch: unscale, then clip_grad_norm_; HipAdam clips inside its step

        def fn():
            if outside:
                scaler.unscale_(opt)
                torch.nn.utils.clip_grad_norm_(params, 1.0)
            scaler.step(opt)
            scaler.update()

        rec[mode] = span(fn, before=lambda: torch._foreach_copy_(grads, scaled if amp else base))
        del opt
        torch.cuda.empty_cache()
    results[name] = rec
    print(name, json.dumps(rec), flush=True)
del model, params, base, scaled, grads
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
    for name in ["none"] + list(BUILD):
        model, params = make_model()
        opt = None if name == "none" else BUILD[name](params)
        at = [0]

        def train_step():
            model.zero_grad(set_to_none=True)
            model.set_training_step(at[0])
            at[0] += 1
            out = model(bundle)
            sum(model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch)).values()).backward()
            if opt is not None:
                opt.step()

        step_rec[name] = span(train_step)
        print("training_step", name, json.dumps(step_rec[name]), flush=True)
        del model, params, opt
        torch.cuda.empty_cache()

doc = {"tool": "tools/optim_bench.py", "device": torch.cuda.get_device_name(0), "parameters": n_params, "reps": a.reps,
       "note": "ms per optimiser step over the default nerfacto's parameters, median and minimum of hipEvent spans, same process; modes: plain "
               "step; scaler: GradScaler.step + update at scale 65536; max_norm: clipping to 1 (torch: clip_grad_norm_ then step, HipAdam: inside "
               "the step); scaler_max_norm: both (torch: unscale_, clip_grad_norm_, step, update).  training_step: the default nerfacto, 4096 "
               "rays, levels (256, 96, 48), training_mlp=\"hip\", forward + losses + backward + the optimiser's plain step (`none`: no optimiser)",
       "results": results, "training_step": step_rec}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", a.out)
