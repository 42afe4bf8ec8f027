"""The mixed-precision MLP on the GPU (``precision="fp16"``: signerf_amd/mlp.py over csrc/sn_mlp_half.h) against tests/mlp_half_oracle.py.

Gates (DESIGN.md §4 "Mixed-precision MLP"):
  integer data  y, dx, every dW_i and db_i equal the fp64 specification bit for bit: nothing rounds and every sum is exact in any order,
                so this is the layout test (the k permutation of two tiles per K-block, the zero-padded K, the [feature][point] images)
  random data   every element of every output within B_flip; the rows of y and of dx with any element beyond 2 x B_tight number at most
                max(1, ceil(0.05 N)) (mlp_half_oracle.bounds; the 2 allows for the matrix instruction's unspecified inner order)
Shapes: the eight stacks of mlp_oracle.STACKS at N = 1, 15..17, 63..65, 1000, 16385 and 32833.  Each test prints its figures before it
asserts.

Measured on an MI355X over the 480 random cases: largest error / B_flip y 0.37, dx 0.50, dW 0.14, db 0.04 (y's bound
carries no mask allowance, and the other three are in cases without a mask-ambiguous element, where B_flip is the plain recursion; 44 418
of 1.72e8 hidden values are marked ambiguous in all); rows above 1 x B_tight at most
1.6 % (y) and 1.4 % (dx) at N >= 1000, one row of 15 at most below that; rms error against the fp32 restatement's, median over the cases
with N >= 1000: y 1.00, dx 0.89, dW 0.82, db 0.70.  The cases at x = 1e-4 (up to 673 951 subnormal hidden values) pass like the others: the
matrix instruction keeps subnormal fp16 operands.  The trainer fit applies 60 steps in 60 iterations (none skipped) and ends at 0.328 of
the initial rgb loss, as the fp32 run of the same process does."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

import mlp_half_oracle as ho
import mlp_oracle as mo
from helpers import ROOT, small_config
from signerf_amd import _lib, mlp
from signerf_amd.nerfacto import MLP

pytestmark = pytest.mark.gpu
D = torch.float64
H = "fp16"
_CASES = {}
_WORST = {}      # output -> (largest error / B_flip, case)
_ROWS = {"y": (0.0, ""), "dx": (0.0, "")}   # largest share of rows above 1 x B_tight
_RMS = {}        # output -> [rms(kernel error) / rms(restatement error) of every case with N >= 1000]


def _to(gpu, *ts):
    return [[t.to(gpu) for t in x] if isinstance(x, list) else x.to(gpu) for x in ts]


def _run(gpu, x, w, b, g, precision=H):
    """-> (y, dx, [dW], [db]) of the two entry points."""
    xg, wg, bg, gg = _to(gpu, x, w, b, g)
    y = mlp.mlp_forward(xg, wg, bg, precision=precision)
    dx, dw, db = mlp.mlp_backward(xg, wg, bg, gg, precision=precision)
    return y, dx, dw, db


def _case(dims, N, wscale, xscale):
    """A random case with its specification, bounds and fp32 restatement, computed once (the small sizes are kept)."""
    key = (dims, N, wscale, xscale)
    if key in _CASES:
        return _CASES[key]
    x, w, b, g = ho.random_case(dims, N, wscale, xscale)
    spec, tight, flip, info = ho.bounds(x, w, b, g)
    r32 = ho.outputs(x, w, b, g, torch.float32)
    case = (x, w, b, g, spec, tight, flip, info, r32)
    if N <= 1000:
        _CASES[key] = case
    return case


def _kind(name):
    return name.rstrip("0123456789")


# ---- 1. exact integer data -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_integer_data_is_exact_bit_for_bit(gpu, dims):
    """No tolerance: a wrong slot of the k permutation, a swapped tile, a K-block or a point of padding that leaks, a partial image that is
    lost shows as a wrong integer."""
    for N in ho.SIZES:
        x, w, b, g = ho.integer_case(dims, N)
        top, terms = ho.integer_case_figures(x, w, b, g)
        assert top <= 2048 and terms < 2.0**24
        want = ho.outputs(x, w, b, g, D)
        got = _run(gpu, x, w, b, g)
        bad = [(name, int((a.double().cpu() != r).sum())) for (name, a), (_, r) in zip(ho.flat(got), ho.flat(want)) if not torch.equal(a.double().cpu(), r)]
        print(f"[half integer] {dims} N={N}: largest rounded value {top:.0f}, sum|terms| {terms:.3g}, wrong elements {bad}")
        assert not bad, (dims, N, bad)


# ---- 2. random data ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xscale", ho.INPUT_SCALES, ids=["x1", "x1e-4", "x30"])
@pytest.mark.parametrize("wscale", ho.WEIGHT_SCALES, ids=["linear_init", "1e-3"])
@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_random_data_meets_both_bounds(gpu, dims, wscale, xscale):
    failed = []
    for N in ho.SIZES:
        x, w, b, g, spec, tight, flip, info, r32 = _case(dims, N, wscale, xscale)
        got = [t.cpu() if isinstance(t, torch.Tensor) else [u.cpu() for u in t] for t in _run(gpu, x, w, b, g)]
        tag = f"{dims} w={'init' if wscale is None else wscale} x={xscale} N={N}"
        line = []
        for (name, a), (_, s), (_, f), (_, r) in zip(ho.flat(got), ho.flat(spec), ho.flat(flip), ho.flat(r32)):
            assert a.shape == s.shape and torch.isfinite(a).all(), (tag, name)
            err = (a.double() - s).abs()
            ratio = float((err / f.clamp_min(1e-300)).max())
            k = _kind(name)
            if ratio > _WORST.get(k, (0.0, ""))[0]:
                _WORST[k] = (ratio, tag)
            e_ref = float((r.double() - s).pow(2).mean().sqrt())
            if e_ref > 0 and N >= 1000:
                _RMS.setdefault(k, []).append(float(err.pow(2).mean().sqrt()) / e_ref)
            line.append(f"{name} {ratio:.3f}")
            if not ratio <= 1.0:
                failed.append((tag, name, "B_flip", ratio))
        for j, k in enumerate(("y", "dx")):
            over1, over2 = ho.rows_above(got[j], spec[j], tight[k], 1.0), ho.rows_above(got[j], spec[j], tight[k], 2.0)
            if over1 / N > _ROWS[k][0]:
                _ROWS[k] = (over1 / N, tag)
            line.append(f"{k} rows>B_tight {over1}, >2B_tight {over2} (cap {ho.row_cap(N)})")
            if over2 > ho.row_cap(N):
                failed.append((tag, k, "rows above 2 x B_tight", over2, ho.row_cap(N)))
        print(f"[half random] {tag}: error / B_flip " + ", ".join(line) + f"; subnormal hidden values {info['subnormal_hidden']}, ambiguous masks "
              f"{info['ambiguous']} of {info['hidden']}, B_flip / plain recursion median {info['inflation']:.4f} largest {info['inflation_max']:.1f}")
    print("[half random] so far: largest error / B_flip " + ", ".join(f"{k} {v[0]:.3f} ({v[1]})" for k, v in _WORST.items()))
    print("[half random] so far: largest share of rows above B_tight " + ", ".join(f"{k} {v[0]:.4f} ({v[1]})" for k, v in _ROWS.items()))
    # (one hidden value that lands on the neighbouring fp16 value, in the kernel or in the restatement, dominates a case's rms: the
    # median over the cases compares the arithmetic, the largest ratio shows such a case)
    print("[half random] so far: rms error / restatement's over the cases with N >= 1000, median and largest: " +
          ", ".join(f"{k} {sorted(v)[len(v) // 2]:.2f} {max(v):.3g}" for k, v in _RMS.items()))
    assert not failed, failed


# ---- 3. edges ------------------------------------------------------------------------------------------------------------------------------
def _raw(gpu, dims, x, w, b, g, N, outs):
    """Both entry points on caller-made buffers: outs = (y, dx, [dW], [db]) are written in place."""
    lib = _lib.load()
    y, dx, dw, db = outs
    ws = torch.empty(mlp.workspace_floats(dims, N), dtype=torch.float32, device=gpu)
    d = mlp._desc(dims, w, b, dw, db, precision=mlp.PRECISIONS[H])
    _lib.check(lib.sn_mlp_forward(C.byref(d), _lib.ptr(x), N, _lib.ptr(y), _lib.current_stream()), None, "sn_mlp_forward")
    _lib.check(lib.sn_mlp_backward(C.byref(d), _lib.ptr(x), _lib.ptr(g), N, _lib.ptr(dx), _lib.ptr(ws), 4 * ws.numel(), _lib.current_stream()),
               None, "sn_mlp_backward")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_rows_past_N_are_neither_read_nor_written(gpu, dims):
    """x and g are the first N rows of buffers whose other rows are NaN; the outputs are the first N rows of sentinel-filled buffers, and the
    parameter gradients sit in the middle of one: the sentinels are intact afterwards, every output is finite and equals the plain call's."""
    S, PAD = -12345.0, 70
    for N in (1, 17, 65, 1000):
        x, w, b, g = _case(dims, N, None, 1.0)[:4]
        xg, wg, bg, gg = _to(gpu, x, w, b, g)
        want = _run(gpu, x, w, b, g)
        xb = torch.full((N + PAD, dims[0]), float("nan"), device=gpu)
        gb = torch.full((N + PAD, dims[-1]), float("nan"), device=gpu)
        xb[:N], gb[:N] = xg, gg
        yb, dxb = torch.full((N + PAD, dims[-1]), S, device=gpu), torch.full((N + PAD, dims[0]), S, device=gpu)
        sizes = [t.numel() for t in wg] + [t.numel() for t in bg]
        pb = torch.full((sum(sizes) + 2 * 8 * len(sizes),), S, device=gpu)     # 8 sentinels on either side of every gradient
        views, at = [], 8
        for t in wg + bg:
            views.append(pb[at:at + t.numel()].view(t.shape))
            at += t.numel() + 16
        dw, db = views[:len(wg)], views[len(wg):]
        _raw(gpu, dims, xb[:N], wg, bg, gb[:N], N, (yb[:N], dxb[:N], dw, db))
        assert bool((yb[N:] == S).all()) and bool((dxb[N:] == S).all()), (dims, N)
        inside = torch.zeros_like(pb, dtype=torch.bool)
        for v in views:
            off = (v.data_ptr() - pb.data_ptr()) // 4
            inside[off:off + v.numel()] = True
        assert bool((pb[~inside] == S).all()) and int((~inside).sum()) == 16 * len(sizes), (dims, N)
        for (name, a), (_, r) in zip(ho.flat((yb[:N], dxb[:N], dw, db)), ho.flat(want)):
            assert torch.isfinite(a).all() and torch.equal(a, r), (dims, N, name)


@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_poisoned_rows_stay_in_their_rows(gpu, dims):
    """NaN, +-inf and 1e30 (beyond fp16: r16 gives inf) in one row of x and 1e6 (the same) in one row of g: every other row of y and dx is
    bit-identical to the clean batch, the two rows are NaN / inf where the restatement's are, and dW / db are non-finite exactly where the
    restatement's are."""
    N, row_x, row_g = 130, 70, 3
    x, w, b, g = [t[:N].clone() if i in (0, 3) else t for i, t in enumerate(_case(dims, 1000, None, 1.0)[:4])]
    clean = _run(gpu, x, w, b, g)
    for j, v in enumerate([float("nan"), float("inf"), -float("inf"), 1e30]):
        x[row_x, j % dims[0]] = v
    g[row_g] = 1e6
    got = _run(gpu, x, w, b, g)
    ref = ho.outputs(x, w, b, g, torch.float32)
    others = (torch.arange(N) != row_x) & (torch.arange(N) != row_g)
    for k, name in enumerate(("y", "dx")):
        a, c, r = got[k].cpu(), clean[k].cpu(), ref[k]
        assert torch.equal(a[others].view(torch.int32), c[others].view(torch.int32)), (name, "another row changed")
        for row in (row_x, row_g):
            print(f"[half poison] {dims} {name}[{row}]: hip {a[row][:6].tolist()} restatement {r[row][:6].tolist()}")
            assert torch.equal(torch.isnan(a[row]), torch.isnan(r[row])) and torch.equal(torch.isinf(a[row]), torch.isinf(r[row])), (name, row)
            assert torch.equal(torch.sign(a[row][torch.isinf(a[row])]), torch.sign(r[row][torch.isinf(r[row])]))
    for (name, a), (_, r) in zip(ho.flat(got)[2:], ho.flat(ref)[2:]):
        assert torch.equal(torch.isfinite(a.cpu()), torch.isfinite(r)), (name, int((~torch.isfinite(a)).sum()), int((~torch.isfinite(r)).sum()))


@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_backward_is_bit_reproducible_and_its_outputs_are_separable(gpu, dims):
    """Two backward calls give the same bits in all outputs (no float atomics); grad_x alone and the parameter gradients alone equal the
    joint call's.  At 65 and 1000 points and at 32833, where every workgroup walks several tiles and 256 partial images are added."""
    for N in (65, 1000, ho.SIZES[-1]):
        x, w, b, g = _case(dims, N, None, 1.0)[:4]
        xg, wg, bg, gg = _to(gpu, x, w, b, g)
        first, second = mlp.mlp_backward(xg, wg, bg, gg, precision=H), mlp.mlp_backward(xg, wg, bg, gg, precision=H)
        only_x = mlp.mlp_backward(xg, wg, bg, gg, want_grad_params=False, precision=H)
        only_w = mlp.mlp_backward(xg, wg, bg, gg, want_grad_x=False, precision=H)
        assert only_x[1] is None and only_x[2] is None and only_w[0] is None
        flat = lambda r: [("dx", r[0])] + [("dW", t) for t in r[1]] + [("db", t) for t in r[2]]   # noqa: E731
        for (name, a), (_, c) in zip(flat(first), flat(second)):
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), (dims, N, name)
        assert torch.equal(first[0].view(torch.int32), only_x[0].view(torch.int32))
        for (name, a), (_, c) in zip(flat(first)[1:], flat((None,) + only_w[1:])[1:]):
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), (dims, N, name)


# ---- 4. precision 0 is untouched -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_fp32_with_and_without_the_argument_gives_the_same_bits(gpu, dims):
    N = 1000
    x, w, b, g = _case(dims, N, None, 1.0)[:4]
    xg, wg, bg, gg = _to(gpu, x, w, b, g)
    res = []
    for kw in ({}, {"precision": "fp32"}):
        xi = xg.clone().requires_grad_()
        ws, bs = [t.clone().requires_grad_() for t in wg], [t.clone().requires_grad_() for t in bg]
        y = mlp.fused_mlp(xi, ws, bs, **kw)
        y.backward(gg)
        res.append([y.detach(), xi.grad] + [t.grad for t in ws + bs] + [mlp.mlp_forward(xg, wg, bg, **kw)] + list(mlp.mlp_backward(xg, wg, bg, gg, **kw)[1]))
    for a, c in zip(*res):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    half = mlp.mlp_forward(xg, wg, bg, precision=H)
    assert not torch.equal(half, res[0][0])        # and the other precision is another arithmetic


# ---- 5. autograd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", mo.REAL_STACKS, ids=str)
def test_autograd_returns_what_the_backward_entry_point_returns(gpu, dims):
    x, w, b, g = _case(dims, 1000, None, 1.0)[:4]
    xg, wg, bg, gg = _to(gpu, x, w, b, g)
    xi = xg.reshape(8, 125, dims[0]).clone().requires_grad_()
    ws, bs = [t.clone().requires_grad_() for t in wg], [t.clone().requires_grad_() for t in bg]
    y = mlp.fused_mlp(xi, ws, bs, precision=H)
    assert y.shape == (8, 125, dims[-1]) and y.requires_grad
    y.backward(gg.reshape(8, 125, dims[-1]))
    want_y = mlp.mlp_forward(xg, wg, bg, precision=H)
    dx, dw, db = mlp.mlp_backward(xg, wg, bg, gg, precision=H)
    assert torch.equal(y.detach().reshape(want_y.shape), want_y) and torch.equal(xi.grad.reshape(dx.shape), dx)
    for t, r in zip(ws + bs, dw + db):
        assert torch.equal(t.grad, r)
    # the module hands its precision over
    m = MLP(dims[0], len(dims) - 1, dims[1], dims[-1], implementation="hip").to(gpu)
    with torch.no_grad():
        for layer, wi, bi in zip(m.layers, wg, bg):
            layer.weight.copy_(wi)
            layer.bias.copy_(bi)
        full = m(xg)
        m.precision = H
        assert torch.equal(m(xg), want_y) and not torch.equal(full, want_y)


# ---- 6. the model --------------------------------------------------------------------------------------------------------------------------
def test_a_training_step_of_the_model_in_mixed_precision(gpu):
    """small_config(training_forward=True, training_mlp="hip", training_mlp_precision="fp16") against the fp32 "hip" model of the same seed:
    every output and every gradient is finite, and the outputs DIFFER (an accidental fp32 run would pass everything else).  The distances
    are printed for DESIGN.md, not gated."""
    import sampler_oracle as so
    from signerf_amd import RayBundle

    R = 256
    o, d, _, _ = so.rays(R, seed=0)
    gen = torch.Generator().manual_seed(0)
    bundle = RayBundle(origins=(0.4 * o).to(gpu), directions=d.to(gpu), pixel_area=torch.ones(R, 1, device=gpu),
                       camera_indices=torch.randint(0, 4, (R, 1), generator=gen).to(gpu))
    batch = {"image": torch.rand(R, 3, generator=gen).to(gpu)}
    outs, models = {}, {}
    for precision in ("fp32", H):
        torch.manual_seed(0)
        model = small_config(training_forward=True, training_mlp="hip", training_mlp_precision=precision, num_train_data=4, camera_optimizer_mode="off",
                             predict_normals=False, use_lpips=False, num_proposal_samples_per_ray=(32, 16), num_nerf_samples_per_ray=12).setup().to(gpu)
        model.train()
        model.set_training_step(0)
        out = model.get_training_outputs(bundle)
        losses_ = model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch))
        sum(losses_.values()).backward()
        outs[precision], models[precision] = out, model
    half, full = models[H], models["fp32"]
    assert [(m.implementation, m.precision) for m in half.modules() if isinstance(m, MLP)] == [("hip", H)] * 4
    for k, v in outs[H].items():
        if isinstance(v, torch.Tensor):
            assert torch.isfinite(v).all(), k
    assert all(torch.isfinite(wl).all() for wl in outs[H]["weights_list"])
    names = lambda m: list(m.field.named_parameters()) + list(m.proposal_networks.named_parameters())   # noqa: E731
    worst = 0.0
    for (n, p), (_, q) in zip(names(half), names(full)):
        assert torch.equal(p.detach(), q.detach()), n
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        top = float(q.grad.abs().max())
        rel = float((p.grad - q.grad).abs().max()) / top if top > 0 else 0.0
        worst = max(worst, rel)
        print(f"[half model] {n}: largest |grad| fp16 {float(p.grad.abs().max()):.3e} fp32 {top:.3e}, largest difference / largest |grad| {rel:.2e}")
    e_rgb = float((outs[H]["rgb"].detach() - outs["fp32"]["rgb"].detach()).abs().max())
    w_h, w_f = outs[H]["weights_list"][-1].detach(), outs["fp32"]["weights_list"][-1].detach()
    print(f"[half model] rendered rgb {e_rgb:.2e} apart, final weights {float((w_h - w_f).abs().max()):.2e}, largest relative gradient distance {worst:.2e}")
    assert e_rgb > 0 and not torch.equal(outs[H]["rgb"], outs["fp32"]["rgb"])


# ---- 7. and 8. the trainer -----------------------------------------------------------------------------------------------------------------
def _trainer_setup(gpu, precision, tmp_path=None):
    """The scene, sizes and optimisers of tests/test_gpu_trainer.py, with the HIP MLP at `precision`."""
    from signerf_amd import Cameras, SIGNeRFDataManager, SIGNeRFDataManagerConfig, scene
    from signerf_amd.config import NerfactoModelConfig
    from signerf_amd.optimizers import AdamOptimizerConfig, ExponentialDecaySchedulerConfig
    from signerf_amd.trainer import Trainer

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_trained_scene as mts

    torch.manual_seed(0)
    Hh = W = 32
    cams = Cameras(scene.benchmark_cameras(4)[:, :3], 40.0, 40.0, W / 2, Hh / 2, W, Hh).to(gpu)
    images = []
    for i in range(4):
        rb = cams.generate_rays(camera_indices=i)
        rgb, _, _ = mts.analytic_image(rb.origins.cpu().reshape(-1, 3), rb.directions.cpu().reshape(-1, 3))
        images.append((rgb.reshape(Hh, W, 3) * 255.0).round().to(torch.uint8))
    images = torch.stack(images).to(gpu)
    dm = SIGNeRFDataManager(SIGNeRFDataManagerConfig(train_num_rays_per_batch=1024), cams, images, generator=torch.Generator(device=gpu).manual_seed(0))
    model = NerfactoModelConfig(log2_hashmap_size=10, num_proposal_samples_per_ray=(16, 8), num_nerf_samples_per_ray=8, num_train_data=4,
                                camera_optimizer_mode="off", training_forward=True, training_mlp="hip", training_mlp_precision=precision,
                                proposal_net_args_list=[{"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 128, "use_linear": False},
                                                        {"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 256, "use_linear": False}]).setup().to(gpu)
    model.train()
    every = torch.stack(torch.meshgrid(torch.arange(4), torch.arange(Hh), torch.arange(W), indexing="ij"), -1).reshape(-1, 3).to(gpu)
    all_rays, all_pixels = dm.train_ray_generator(every)
    config = {k: {"optimizer": AdamOptimizerConfig(lr=1e-2, eps=1e-15, max_norm=1.0, implementation="hip"),
                  "scheduler": ExponentialDecaySchedulerConfig(lr_final=1e-4, max_steps=200000)} for k in ("proposal_networks", "fields", "camera_opt")}
    trainer = Trainer(model, dm, config, mixed_precision=True)

    def whole_loss():
        with torch.no_grad():
            return float(model.get_loss_dict(model(all_rays), {"image": all_pixels})["rgb_loss"])

    return trainer, model, whole_loss


def _fit(trainer, model, whole_loss, applied_wanted=60, cap=90):
    """-> (ratio of the rgb loss over all pixels, iterations, skipped, applied): runs until `applied_wanted` steps have been applied.  A step
    is applied if it changed the colour head's output bias, which has a gradient in every iteration; a skipped step changes no parameter."""
    watched = model.field.mlp_head.layers[-1].bias
    first, applied, it = whole_loss(), 0, 0
    while applied < applied_wanted and it < cap:
        before = watched.detach().clone()
        loss, _, _ = trainer.train_iteration(it)
        it += 1
        applied += not torch.equal(before, watched.detach())
    return whole_loss() / first, it, it - applied, applied


def test_the_references_configuration_fits_the_analytic_scene(gpu):
    """training_mlp_precision="fp16" under Trainer(mixed_precision=True) with the HIP Adam, on the scene, sizes and 1024-ray steps of
    test_a_training_loop_fits_an_analytic_scene: until 60 steps have been APPLIED, in at most 90 iterations; the rgb loss over all 4096
    pixels ends below half the initial one, and the scale is finite and positive.  The fp32 run of the same process is printed beside it."""
    trainer, model, whole_loss = _trainer_setup(gpu, H)
    assert [m.precision for m in model.modules() if isinstance(m, MLP)] == [H] * 4 and trainer.grad_scaler.is_enabled()
    ratio, iterations, skipped, applied = _fit(trainer, model, whole_loss)
    scale = trainer.grad_scaler.get_scale()
    trainer32, model32, whole_loss32 = _trainer_setup(gpu, "fp32")
    ratio32, iterations32, skipped32, _ = _fit(trainer32, model32, whole_loss32)
    print(f"\n[half trainer] fp16: rgb loss ratio {ratio:.3f} after {iterations} iterations, {skipped} skipped, grad scale {scale}; "
          f"fp32: {ratio32:.3f} after {iterations32} iterations, {skipped32} skipped")
    assert applied == 60 and iterations <= 90
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert ratio < 0.5
    assert math.isfinite(scale) and scale > 0


def test_an_overflowing_gradient_skips_the_step_and_halves_the_scale(gpu):
    """One Trainer step whose loss scale (2^50) pushes r16(g) beyond fp16's range -- an arithmetic overflow on valid memory: a gradient is
    non-finite, no parameter changes in any bit, and the scale has halved."""
    trainer, model, _ = _trainer_setup(gpu, H)
    trainer.grad_scaler = torch.amp.GradScaler("cuda", init_scale=2.0**50, enabled=True)
    before = [p.detach().clone() for p in model.parameters()]
    trainer.train_iteration(0)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and any(not torch.isfinite(gr).all() for gr in grads)
    assert all(torch.equal(a.view(torch.int32), p.detach().view(torch.int32)) for a, p in zip(before, model.parameters()) if p.numel())
    assert trainer.grad_scaler.get_scale() == 2.0**49
