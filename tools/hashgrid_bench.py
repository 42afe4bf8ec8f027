#!/usr/bin/env python3
"""What the trainable hash grid costs (signerf_amd/hashgrid.py over csrc/sn_hashgrid.h) beside the same encoding as plain torch ops with
autograd (oracle.nerfacto.hash_encode in fp32) on the same GPU, in the same process.  Recorded, not gated (DESIGN.md §4 "Trainable hash grid").

Shapes: the three grids of a nerfacto step at 4096 rays -- the main field (48 samples, 16 levels, T = 2^19, max_res 2048) and the two
proposal nets (256 and 96 samples, 5 levels, T = 2^17, max_res 128 and 256).  The points are consecutive samples along rays through the
contracted scene, in ray-major order as training produces them (the wave merge of the table gradient depends on that order; i.i.d. points
would not show it): origins on a sphere of radius 1.2 looking at the unit ball, stratified samples in nerfacto's piecewise spacing between
0.05 and 1000, contracted and mapped to [0, 1].

Per shape, forward + backward (table gradient, zeroing it included), the median of 50 hipEvent spans after a warm-up:
  hip_a        the plain table gradient, one atomic add per corner and feature (SN_HASHGRID_MERGE_MAX_SCALE=-1)
  hip_shipped  the library's default
  hip_merge_upto[k]  equal rows merged within the wave on the levels 0..k, plain above (the sweep the shipped threshold is read from)
  torch        oracle.nerfacto.hash_encode, fp32 torch ops with autograd
and beside them what the bytes the table gradient adds would cost at the guide's two float-atomic rates (scattered rows, contiguous).

    python tools/hashgrid_bench.py [--reps 50] [--out profiles/hashgrid_bench.json]

``--grid tcnn`` measures the trainable tiny-cuda-nn grid (hashgrid.hash_encode(grid="tcnn"), csrc/sn_hashgrid_tcnn.h; DESIGN.md §4
"Trainable tcnn grid") on the same shapes and points, with the library's own scales and its dense coarse levels, and writes
profiles/hashgrid_tcnn_bench.json.  Its reference, in the same process, is the torch-path grid's kernels at their shipped threshold
(``torch_grid_shipped``) instead of the torch ops; each record names the dense levels.

``--table-grad ordered`` (with either ``--grid``) times the two forms of the table gradient against each other instead: the shipped atomics
and the ordered, bit-reproducible sum (``hash_encode(table_grad="ordered")``, csrc/sn_hashgrid_ordered.h; DESIGN.md §4 "Ordered table
gradient") on the same three shapes, then one whole training step with ``config.training_hashgrid_grad`` set each way, and writes
profiles/hashgrid_ordered_bench.json (``--grid tcnn``: hashgrid_ordered_tcnn_bench.json) with the workspace sizes.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from oracle import nerfacto as onf  # noqa: E402
from oracle import tcnn_layout  # noqa: E402
from signerf_amd import _lib, hashgrid  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=4096)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--no-sweep", action="store_true")
ap.add_argument("--grid", choices=("torch", "tcnn"), default="torch")
ap.add_argument("--table-grad", choices=("atomic", "ordered"), default="atomic")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if a.table_grad == "ordered":
    a.out = a.out or os.path.join(ROOT, "profiles", "hashgrid_ordered_bench.json" if a.grid == "torch" else "hashgrid_ordered_tcnn_bench.json")
a.out = a.out or os.path.join(ROOT, "profiles", "hashgrid_bench.json" if a.grid == "torch" else "hashgrid_tcnn_bench.json")
dev = torch.device("cuda", 0)
ENV = "SN_HASHGRID_MERGE_MAX_SCALE"
SHAPES = {"main": dict(samples=48, L=16, log2_T=19, base=16, max_res=2048), "proposal_0": dict(samples=256, L=5, log2_T=17, base=16, max_res=128),
          "proposal_1": dict(samples=96, L=5, log2_T=17, base=16, max_res=256)}
SCATTERED_TBPS, CONTIGUOUS_TBPS = 0.08, 1.3   # float atomic adds: 64 lanes into 64 rows / 256 contiguous bytes per wave instruction


def ray_points(R, S, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 1.2
    look = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * torch.rand(R, 1, generator=g) ** (1 / 3)
    d = torch.nn.functional.normalize(look - o, dim=-1)
    s = (torch.arange(S)[None, :] + torch.rand(R, S, generator=g)) / S
    t = onf.spacing_to_euclidean(s, torch.full((R, 1), 0.05), torch.full((R, 1), 1000.0))
    q, _ = onf.normalized_positions(o[:, None, :] + d[:, None, :] * t[..., None])
    return q.reshape(-1, 3).contiguous()


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


def set_merge(value):
    if value is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = repr(float(value))
    _lib.check(_lib.load().sn_hashgrid_debug_reload_env(), None, "sn_hashgrid_debug_reload_env")


def ordered_ab():
    """--table-grad ordered: both forms of the table gradient (hashgrid.hash_encode(table_grad=...)) on the three shapes, forward + backward
    with the zeroing of grad_table, then one whole training step of the default nerfacto with config.training_hashgrid_grad set each way."""
    from signerf_amd.cameras import RayBundle
    from signerf_amd.config import NerfactoModelConfig

    lib = _lib.load()
    results = {}
    for name, sh in SHAPES.items():
        L, log2_T = sh["L"], sh["log2_T"]
        q = ray_points(a.rays, sh["samples"], seed=len(name)).to(dev)
        meta = tcnn_layout.grid_meta(L, sh["base"], sh["max_res"], log2_T) if a.grid == "tcnn" else None
        s_dev = (onf.hash_scalings(L, sh["base"], sh["max_res"]) if meta is None else torch.tensor(meta.scales, dtype=torch.float32)).to(dev)
        table = ((torch.rand((L << log2_T, 2), generator=torch.Generator().manual_seed(1)) * 2 - 1) * 1e-3).to(dev).requires_grad_()
        g = torch.randn(q.shape[0], L * 2, generator=torch.Generator().manual_seed(2)).to(dev)

        def step(form):
            table.grad = None
            hashgrid.hash_encode(q, table, s_dev, log2_T, grid=a.grid, table_grad=form).backward(g)

        def forward():
            with torch.no_grad():
                hashgrid.hash_encode(q, table, s_dev, log2_T, grid=a.grid)

        rec = {"points": q.shape[0], "levels": L, "log2_T": log2_T, "contributions_per_level": q.shape[0] * 8,
               "workspace_bytes": lib.sn_hashgrid_ordered_workspace_bytes(q.shape[0], L, log2_T, 2), "radix_passes": (log2_T + 7) // 8,
               "launches_per_backward": L * (2 + 3 * ((log2_T + 7) // 8))}
        rec["hip_forward"] = span(forward)
        rec["atomic"] = span(lambda: step("atomic"))
        rec["ordered"] = span(lambda: step("ordered"))
        rec["ordered_over_atomic"] = round(rec["ordered"]["ms_median"] / rec["atomic"]["ms_median"], 2)
        step("ordered")
        first = table.grad.clone()
        step("ordered")
        rec["ordered_bits_repeat"] = bool(torch.equal(first.view(torch.int32), table.grad.view(torch.int32)))
        step("atomic")
        rec["largest_difference_to_atomic"] = float((table.grad - first).abs().max())
        results[name] = rec
        print(name, json.dumps(rec), flush=True)
        del table, q, g, first
        torch.cuda.empty_cache()
    R = a.rays
    gen = torch.Generator().manual_seed(0)
    o = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * 0.5
    look = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * 0.2
    bundle = RayBundle(origins=o.to(dev), directions=torch.nn.functional.normalize(look - o, dim=-1).to(dev), pixel_area=torch.ones(R, 1, device=dev),
                       camera_indices=torch.randint(0, 4, (R, 1), generator=gen).to(dev))
    batch = {"image": torch.rand(R, 3, generator=gen).to(dev)}
    kw = dict(implementation="tcnn", training_tcnn=True) if a.grid == "tcnn" else {}
    step_rec = {}
    for form in ("atomic", "ordered"):
        torch.manual_seed(0)
        model = NerfactoModelConfig(training_forward=True, training_mlp="hip", training_hashgrid_grad=form, num_train_data=4,
                                    camera_optimizer_mode="off", **kw).setup().to(dev)
        model.train()
        at = [0]

        def train_step():
            model.zero_grad(set_to_none=True)
            model.set_training_step(at[0])
            at[0] += 1
            out = model(bundle)
            sum(model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch)).values()).backward()

        step_rec[form] = span(train_step)
        print("training_step", form, json.dumps(step_rec[form]), flush=True)
        del model
        torch.cuda.empty_cache()
    step_rec["ordered_over_atomic"] = round(step_rec["ordered"]["ms_median"] / step_rec["atomic"]["ms_median"], 2)
    return {"tool": "tools/hashgrid_bench.py --table-grad ordered", "grid": a.grid, "device": torch.cuda.get_device_name(0), "rays": a.rays, "reps": a.reps,
            "note": "forward + backward (table gradient, its zeroing and, for `ordered`, the allocation of its workspace included) per call, ms, median of "
                    "hipEvent spans, both forms in the same process on the same points; `atomic` is the library's default (merged atomics at its "
                    "shipped threshold); `training_step`: the default nerfacto, training_mlp=\"hip\", 4096 rays, levels (256, 96, 48), forward + "
                    "losses + backward, no optimiser, config.training_hashgrid_grad set each way",
            "results": results, "training_step": step_rec}


def write(doc):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if a.table_grad == "ordered":
    write(ordered_ab())
    sys.exit(0)

results = {}
for name, sh in SHAPES.items():
    L, log2_T = sh["L"], sh["log2_T"]
    q = ray_points(a.rays, sh["samples"], seed=len(name)).to(dev)
    s_torch = onf.hash_scalings(L, sh["base"], sh["max_res"])
    meta = tcnn_layout.grid_meta(L, sh["base"], sh["max_res"], log2_T) if a.grid == "tcnn" else None
    s = s_torch if meta is None else torch.tensor(meta.scales, dtype=torch.float32)
    s_dev, s_torch_dev = s.to(dev), s_torch.to(dev)
    table = ((torch.rand((L << log2_T, 2), generator=torch.Generator().manual_seed(1)) * 2 - 1) * 1e-3).to(dev).requires_grad_()
    g = torch.randn(q.shape[0], L * 2, generator=torch.Generator().manual_seed(2)).to(dev)

    def hip_forward():
        with torch.no_grad():
            hashgrid.hash_encode(q, table, s_dev, log2_T, grid=a.grid)

    def hip_step():
        table.grad = None
        hashgrid.hash_encode(q, table, s_dev, log2_T, grid=a.grid).backward(g)

    def torch_grid_step():
        table.grad = None
        hashgrid.hash_encode(q, table, s_torch_dev, log2_T).backward(g)

    def torch_step():
        table.grad = None
        onf.hash_encode(q, table, s_dev, log2_T).backward(g)

    added = q.shape[0] * L * 8 * 2 * 4
    rec = {"points": q.shape[0], "levels": L, "log2_T": log2_T, "scalings": s.tolist(), "grad_table_bytes_added": added,
           "atomic_rate_ms": {"scattered_0.08_TBps": round(added / (SCATTERED_TBPS * 1e9), 3), "contiguous_1.3_TBps": round(added / (CONTIGUOUS_TBPS * 1e9), 3)}}
    if meta is not None:
        rec["dense_levels"] = [l for l in range(L) if meta.dense[l]]
        rec["level_rows"] = [meta.offsets[l + 1] - meta.offsets[l] for l in range(L)]
    rec["hip_forward"] = span(hip_forward)
    set_merge(-1.0)
    rec["hip_a"] = span(hip_step)
    if not a.no_sweep:
        rec["hip_merge_upto"] = []
        for k in range(L):
            set_merge(s[k].item())
            rec["hip_merge_upto"].append(dict(level=k, max_scale=s[k].item(), **span(hip_step)))
    set_merge(None)
    rec["hip_shipped"] = span(hip_step)
    if a.grid == "tcnn":
        rec["torch_grid_shipped"] = span(torch_grid_step)
        rec["tcnn_over_torch_grid"] = round(rec["hip_shipped"]["ms_median"] / rec["torch_grid_shipped"]["ms_median"], 2)
    else:
        rec["torch"] = span(torch_step)
        rec["torch_over_hip_shipped"] = round(rec["torch"]["ms_median"] / rec["hip_shipped"]["ms_median"], 2)
    results[name] = rec
    print(name, json.dumps(rec), flush=True)
    del table, q, g
    torch.cuda.empty_cache()

doc = {"tool": "tools/hashgrid_bench.py", "grid": a.grid, "device": torch.cuda.get_device_name(0), "rays": a.rays, "reps": a.reps,
       "note": "forward + backward (table gradient) per call, ms, median of hipEvent spans; `torch`: oracle.nerfacto.hash_encode as fp32 torch "
               "ops with autograd on the same GPU in the same process; `torch_grid_shipped` (--grid tcnn): the torch-path grid's kernels "
               "on the same points, table and process; points are ray-ordered samples through the contracted scene",
       "results": results}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", a.out)
