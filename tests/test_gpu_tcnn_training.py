"""Fine-tuning a tiny-cuda-nn field on the GPU (``config.training_tcnn``): the training paths of an imported checkpoint's fields against
the oracle's tcnn field (``oracle.nerfacto`` with its tcnn grid and SH remap, on ``oracle_params_from_tcnn``), the same on the fused HIP
MLP, a backward pass and an optimiser step followed by an eval render of the updated parameters, and the end-to-end fit of
tests/test_gpu_sampler.py::test_a_training_loop_fits_an_analytic_scene on a tcnn model.

Gates are the ones the torch-path tests apply to the same quantities: the training forward's (tests/test_gpu_sampler.py: density 1e-4
relative, geo 2e-5 of max(scale, 1), rgb 2e-5), the torch / hip model pair's (tests/test_gpu_mlp.py: rendered and field rgb 2e-5, densities
1e-4 relative), the tcnn eval render's (tests/test_gpu_tcnn.py: rmse 1e-3) and the fit's (final loss below half the initial one).  Every
test prints its figures before it asserts."""
import pytest
import torch

import sampler_oracle as so
import tcnn_hashgrid_oracle as to
from helpers import oracle_config, oracle_params_from_tcnn, rmse, small_config, synthetic_tcnn_checkpoint
from oracle import nerfacto as onf
from oracle import tcnn_layout as tl
from signerf_amd import Cameras, FieldHeadNames, Frustums, RayBundle, RaySamples, samplers, scene
from signerf_amd.nerfacto import MLP, HashEncoding

pytestmark = pytest.mark.gpu


def _config(**kw):
    """A tcnn model that trains; opacity as tests/test_gpu_tcnn.py sets it (the checkpoint's nets are bias-free), no LPIPS weights."""
    base = dict(implementation="tcnn", training_tcnn=True, training_forward=True, camera_optimizer_mode="off", average_init_density=3.0,
                use_lpips=False)
    base.update(kw)
    return small_config(**base)


def _model(gpu, cfg, sd):
    model = cfg.setup()
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    return model.to(gpu).train()


def _grids(cfg):
    """(prefix, level table) of the model's three grids."""
    out = [("field.mlp_base", tl.grid_meta(cfg.num_levels, cfg.base_res, cfg.max_res, cfg.log2_hashmap_size))]
    for i in range(cfg.num_proposal_iterations):
        a = cfg.proposal_net_args_list[i]
        out.append((f"proposal_networks.{i}.mlp_base", tl.grid_meta(a["num_levels"], a.get("base_res", 16), a["max_res"], a["log2_hashmap_size"])))
    return out


def _oracle_params(model, cfg):
    """The model's CURRENT parameters in the oracle's layout: its state dict, the uniform tables back in the library's row order."""
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for prefix, meta in _grids(cfg):
        params[f"{prefix}.encoder.tcnn_grid"] = to.flat_rows(params[f"{prefix}.encoder.hash_table"], meta)
    return params


def _bundle(gpu, R, seed=0):
    o, d, _, _ = so.rays(R, seed=seed)
    g = torch.Generator().manual_seed(seed)
    b = RayBundle(origins=(0.4 * o).to(gpu), directions=d.to(gpu), pixel_area=torch.ones(R, 1, device=gpu),
                  camera_indices=torch.randint(0, 4, (R, 1), generator=g).to(gpu))
    return b, {"image": torch.rand(R, 3, generator=g).to(gpu)}


def _samples(gpu, R=37, S=11):
    """A sampler's own samples (the kernel's q / selector) and samples from elsewhere (torch-op positions, far ones included), as
    tests/test_gpu_sampler.py::test_training_paths_of_the_fields_match_the_hip_stage has them."""
    b, _ = _bundle(gpu, R, seed=R)
    from_sampler = samplers.sample_initial(b, S, single_jitter=False, seed=3)
    g = torch.Generator().manual_seed(0)
    o = (torch.rand(R, 1, 3, generator=g) - 0.5).expand(R, S, 3).contiguous()
    d = torch.nn.functional.normalize(torch.randn(R, 1, 3, generator=g), dim=-1).expand(R, S, 3).contiguous()
    bins = torch.cumsum(torch.rand(R, S + 1, 1, generator=g) * 0.4, dim=1)
    bins[:3] *= 30.0
    elsewhere = RaySamples(Frustums(o.to(gpu), d.to(gpu), bins[:, :-1].to(gpu), bins[:, 1:].to(gpu), torch.ones(R, S, 1, device=gpu)))
    return from_sampler, elsewhere


def _rel(got, want):
    return float(((got - want).abs() / want.clamp_min(1e-6)).max())


@pytest.fixture(scope="module")
def checkpoint():
    cfg = _config()
    sd = synthetic_tcnn_checkpoint(cfg, seed=0)
    return sd, oracle_params_from_tcnn(sd, cfg)


def test_training_paths_of_the_fields_match_the_oracles_tcnn_field(gpu, checkpoint):
    sd, params = checkpoint
    cfg = _config()
    model = _model(gpu, cfg, sd)
    assert all(m.trainable_tcnn for m in model.modules() if isinstance(m, HashEncoding))
    ocfg = oracle_config(cfg)
    assert ocfg.sh_remap == "tcnn" and ocfg.main.grid == "tcnn"
    for rs in _samples(gpu):
        pos, dirs = rs.frustums.get_positions().cpu(), rs.frustums.directions[:, 0].cpu()
        R, S = pos.shape[:2]
        o_d, h, _, _ = onf.density_field(params, "field.mlp_base", ocfg.main, pos, ocfg.average_init_density)
        o_rgb, o_geo = onf.field_rgb(params, ocfg, dirs, h), h[..., 1:16]
        out = model.field.forward_training(rs, appearance="mean", return_geo=True)
        density, rgb, geo = out[FieldHeadNames.DENSITY], out[FieldHeadNames.RGB], out["geo"]
        assert density.shape == (R, S, 1) and rgb.shape == (R, S, 3) and geo.shape == (R, S, 15) and density.requires_grad and rgb.requires_grad
        e_d = _rel(density.detach().cpu(), o_d)
        scale = float(o_geo.abs().max())
        e_g, e_c = float((geo.detach().cpu() - o_geo).abs().max()), float((rgb.detach().cpu() - o_rgb).abs().max())
        e_p = []
        for i, net in enumerate(model.proposal_networks):
            o_p, _, _, _ = onf.density_field(params, f"proposal_networks.{i}.mlp_base", ocfg.proposals[i], pos, ocfg.average_init_density)
            di = net.get_density_training(rs)
            assert di.shape == (R, S, 1) and di.requires_grad
            e_p.append(_rel(di.detach().cpu(), o_p))
        print(f"\n[tcnn training path] density rel {e_d:.2e}  geo {e_g:.2e} (scale {scale:.2f})  rgb {e_c:.2e}  proposal densities rel "
              f"{e_p[0]:.2e} {e_p[1]:.2e}  (oracle rgb std {float(o_rgb.std()):.3f}, density in [{float(o_d.min()):.2e}, {float(o_d.max()):.2e}])")
        assert float(o_rgb.std()) > 0.05 and float(o_d.max()) > 0
        assert e_d <= 1e-4 and e_g <= 2e-5 * max(scale, 1.0) and e_c <= 2e-5
        assert max(e_p) <= 1e-4
    with pytest.raises(NotImplementedError):
        model.field.forward_training(rs, compute_normals=True)


def test_the_model_on_the_hip_mlp_matches_the_model_on_torch_ops(gpu, checkpoint):
    """The pair of tests/test_gpu_mlp.py::test_a_training_step_of_the_model_on_the_hip_mlp, on the imported tcnn checkpoint; and one
    mixed-precision step, which has to leave finite gradients."""
    sd, _ = checkpoint
    R = 256
    bundle, batch = _bundle(gpu, R)
    kw = dict(num_train_data=50, num_proposal_samples_per_ray=(32, 16), num_nerf_samples_per_ray=12)
    outs, models = {}, {}
    for impl in ("torch", "hip"):
        model = _model(gpu, _config(training_mlp=impl, **kw), sd)
        model.set_training_step(0)
        out = model.get_training_outputs(bundle)
        sum(model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch)).values()).backward()
        outs[impl], models[impl] = out, model
    hip = models["hip"]
    assert [m.implementation for m in hip.modules() if isinstance(m, MLP)] == ["hip"] * 5     # (base, head, pred normals, two proposal nets)
    names = lambda m: [(n, p) for n, p in list(m.field.named_parameters()) + list(m.proposal_networks.named_parameters())  # noqa: E731
                       if "pred_normals" not in n and "embedding" not in n]
    for (n, p), (_, q) in zip(names(hip), names(models["torch"])):
        assert torch.equal(p.detach(), q.detach()), n
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        top_h, top_t = float(p.grad.abs().max()), float(q.grad.abs().max())
        print(f"[tcnn mlp model] {n}: largest |grad| hip {top_h:.3e} torch {top_t:.3e}, largest difference {float((p.grad - q.grad).abs().max()):.2e}")
        assert (top_h > 0) == (top_t > 0), n
    e_rgb = float((outs["hip"]["rgb"].detach() - outs["torch"]["rgb"].detach()).abs().max())
    rs = outs["torch"]["ray_samples_list"][-1]
    with torch.no_grad():
        f = {impl: models[impl].field.forward_training(rs) for impl in models}
        p = {impl: [net.get_density_training(rs) for net in models[impl].proposal_networks] for impl in models}
    e_d = _rel(f["hip"][FieldHeadNames.DENSITY], f["torch"][FieldHeadNames.DENSITY])
    e_c = float((f["hip"][FieldHeadNames.RGB] - f["torch"][FieldHeadNames.RGB]).abs().max())
    e_p = max(_rel(a, b) for a, b in zip(p["hip"], p["torch"]))
    print(f"[tcnn mlp model] rendered rgb {e_rgb:.2e}; field rgb {e_c:.2e}, density rel {e_d:.2e}, proposal density rel {e_p:.2e}")
    assert e_rgb <= 2e-5 and e_c <= 2e-5 and e_d <= 1e-4 and e_p <= 1e-4
    half = _model(gpu, _config(training_mlp="hip", training_mlp_precision="fp16", **kw), sd)
    half.set_training_step(0)
    out = half.get_training_outputs(bundle)
    sum(half.get_loss_dict(out, batch, half.get_metrics_dict(out, batch)).values()).backward()
    e_half = float((out["rgb"].detach() - outs["torch"]["rgb"].detach()).abs().max())
    print(f"[tcnn mlp model] fp16: rendered rgb against the torch model {e_half:.2e}")
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for _, p in names(half)) and bool(torch.isfinite(out["rgb"]).all())


def test_a_step_reaches_every_parameter_and_the_eval_render_follows(gpu, checkpoint):
    """backward(): a gradient on the three tables -- exactly 0 on the rows no level can address -- and on every stack of the training
    forward; then one Adam step, ``mark_weights_dirty()`` and an eval render of a 24 x 24 frame against the oracle on the UPDATED
    parameters, under the gates of tests/test_gpu_tcnn.py."""
    sd, before = checkpoint
    cfg = _config()
    model = _model(gpu, cfg, sd)
    bundle, batch = _bundle(gpu, 256)
    model.set_training_step(0)
    out = model(bundle)                                   # training_forward=True and train(): get_training_outputs
    assert "weights_list" in out and out["rgb"].requires_grad
    sum(model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch)).values()).backward()
    unused = 0
    for prefix, meta in _grids(cfg):
        grad = model.get_parameter(f"{prefix}.encoder.hash_table").grad
        used = to.used_rows(meta)                         # (the proposal nets' one dense level, r = 16 at T = 2^12, fills its slot)
        unused += int((~used).sum())
        assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0, prefix
        assert bool((grad.cpu()[~used] == 0).all()), prefix
        for name, p in model.get_submodule(f"{prefix}.mlp").named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (prefix, name)
    assert unused > 0                                     # the main grid's two dense levels leave most of their slots unused
    for name, p in model.field.mlp_head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    opt = torch.optim.Adam([p for p in model.parameters() if p.grad is not None], lr=1e-2, eps=1e-15)
    opt.step()
    model.mark_weights_dirty()                            # the optimiser wrote the parameters in place
    params = _oracle_params(model, cfg)
    moved = float((params["field.mlp_base.encoder.tcnn_grid"] - before["field.mlp_base.encoder.tcnn_grid"]).abs().max())
    bias = float(params["field.mlp_base.mlp.layers.1.bias"].abs().max())
    assert moved > 1e-3 and bias > 1e-3                   # the imported zero biases are ordinary parameters: they train
    model.eval()
    H = W = 24
    b = Cameras(scene.benchmark_cameras(8)[:, :3], 30.0, 30.0, W / 2, H / 2, W, H).to(gpu)[2].generate_rays(0)
    got = model.get_outputs_for_camera_ray_bundle(b)
    ref = onf.get_outputs_for_camera_ray_bundle(params, oracle_config(cfg), b.origins.cpu(), b.directions.cpu())
    stale = onf.get_outputs_for_camera_ray_bundle(before, oracle_config(cfg), b.origins.cpu(), b.directions.cpu())
    e = {k: rmse(got[k], ref[k]) for k in ("rgb", "depth", "accumulation")}
    print(f"\n[tcnn step then eval render] table moved by {moved:.2e}, largest base bias {bias:.2e};", {k: f"{v:.2e}" for k, v in e.items()},
          f"; the render of the parameters BEFORE the step is {rmse(stale['rgb'], ref['rgb']):.2e} away in rgb")
    assert all(v <= 1e-3 for v in e.values()), e
    assert float(ref["rgb"].std()) > 0.05 and rmse(stale["rgb"], ref["rgb"]) > 1e-3      # non-vacuous: the step is visible


def test_a_training_loop_fits_an_analytic_scene_on_a_tcnn_model(gpu):
    """tests/test_gpu_sampler.py::test_a_training_loop_fits_an_analytic_scene with implementation="tcnn": the same 4 cameras of 32 x 32,
    table sizes, 60 Adam steps and learning rate, from a fresh initialisation; the same gate (DESIGN.md §4 "Trainable tcnn grid" records
    the measured ratio beside the torch path's 0.33)."""
    import os
    import sys

    from helpers import ROOT
    from signerf_amd import SIGNeRFDataManager, SIGNeRFDataManagerConfig
    from signerf_amd.config import NerfactoModelConfig

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_trained_scene as mts

    torch.manual_seed(0)
    H = W = 32
    cams = Cameras(scene.benchmark_cameras(4)[:, :3], 40.0, 40.0, W / 2, H / 2, W, H).to(gpu)
    images = []
    for i in range(4):
        rb = cams.generate_rays(camera_indices=i)
        rgb, _, _ = mts.analytic_image(rb.origins.cpu().reshape(-1, 3), rb.directions.cpu().reshape(-1, 3))
        images.append((rgb.reshape(H, W, 3) * 255.0).round().to(torch.uint8))
    images = torch.stack(images).to(gpu)
    dm = SIGNeRFDataManager(SIGNeRFDataManagerConfig(train_num_rays_per_batch=1024), cams, images,
                            generator=torch.Generator(device=gpu).manual_seed(0))
    cfg = NerfactoModelConfig(log2_hashmap_size=10, num_proposal_samples_per_ray=(16, 8), num_nerf_samples_per_ray=8, num_train_data=4,
                              camera_optimizer_mode="off", training_forward=True, implementation="tcnn", training_tcnn=True,
                              proposal_net_args_list=[{"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 128, "use_linear": False},
                                                      {"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 256, "use_linear": False}])
    model = cfg.setup().to(gpu)
    model.train()
    every = torch.stack(torch.meshgrid(torch.arange(4), torch.arange(H), torch.arange(W), indexing="ij"), -1).reshape(-1, 3).to(gpu)
    all_rays, all_pixels = dm.train_ray_generator(every)

    def whole_loss():
        with torch.no_grad():
            return float(model.get_loss_dict(model(all_rays), {"image": all_pixels})["rgb_loss"])

    first = whole_loss()
    opt = torch.optim.Adam([p for p in model.parameters() if p.numel()], lr=1e-2, eps=1e-15)
    for step in range(60):
        model.set_training_step(step)
        bundle, batch = dm.next_train(step)
        out = model(bundle)
        loss = sum(model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch)).values())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    final = whole_loss()
    print(f"\n[tcnn training fit] rgb loss {first:.5f} -> {final:.5f} ({final / first:.3f} of the initial)")
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert final < 0.5 * first
    model.mark_weights_dirty()
    model.eval()
    assert torch.isfinite(model(all_rays.get_row_major_sliced_ray_bundle(0, 64))["rgb"]).all()
