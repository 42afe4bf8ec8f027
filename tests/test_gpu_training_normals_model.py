"""Training-mode normals through the field and the model (config.training_normals; DESIGN.md §4 "Training-mode normals"):
``NerfactoField.forward_training(compute_normals=True)`` against ``oracle.nerfacto.field_analytic_normals`` / ``field_pred_normals`` on
the module's own parameters, one training step of a ``predict_normals`` model through the loss dict and ``backward()`` on both MLP
implementations, and the flag's off state.

The field's gates are the ones tests/test_gpu_normals_samples.py applies to the eval kernel: normals_oracle.gate (factor 8) against the
fp64 restatement of tests/normals_oracle.py, e_ref32 the oracle's own error, on the samples no tie decides (normals_oracle.ambiguous: a
ReLU tie or a position within 2 ulp of a voxel face; at most 2 %).  Figures are printed before they are asserted."""
import dataclasses

import pytest
import torch

import normals_oracle as no
import sampler_oracle as so
from helpers import make_model, onf, oracle_config, small_config
from signerf_amd import FieldHeadNames, RayBundle, samplers
from signerf_amd.nerfacto import MLP

pytestmark = pytest.mark.gpu
BASE_KEYS = {"rgb", "accumulation", "depth", "expected_depth", "weights_list", "ray_samples_list", "prop_depth_0", "prop_depth_1"}
NEW_KEYS = {"normals", "pred_normals", "rendered_orientation_loss", "rendered_pred_normal_loss"}


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(gpu):
    """A device error ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize(gpu)
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _tiny_config(**kw):
    """tests/test_gpu_sampler.py::_tiny_config's values: tables of 2^10 rows, levels of (16, 8, 8) samples."""
    from signerf_amd.config import NerfactoModelConfig

    base = dict(log2_hashmap_size=10, num_proposal_samples_per_ray=(16, 8), num_nerf_samples_per_ray=8, num_train_data=4,
                camera_optimizer_mode="off", training_forward=True,
                proposal_net_args_list=[{"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 128, "use_linear": False},
                                        {"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 256, "use_linear": False}])
    base.update(kw)
    return NerfactoModelConfig(**base)


# ---- the field -----------------------------------------------------------------------------------------------------------------------------
def test_field_normals_match_the_oracle_on_the_modules_own_parameters(gpu):
    cfg = small_config(precision="fp32", predict_normals=True, training_normals=True)
    model, _ = make_model(cfg, gpu)
    R, S = 37, 11
    o, d, nears, fars = so.rays(R, seed=R)
    b = RayBundle(origins=o.to(gpu), directions=d.to(gpu), pixel_area=torch.ones(R, 1, device=gpu),
                  camera_indices=torch.arange(R, device=gpu)[:, None] % 4, nears=nears[:, None].to(gpu), fars=fars[:, None].to(gpu))
    rs = samplers.sample_initial(b, S, single_jitter=False, seed=3)
    out = model.field.forward_training(rs, appearance="mean", compute_normals=True)
    normals, pred = out[FieldHeadNames.NORMALS], out[FieldHeadNames.PRED_NORMALS]
    assert normals.shape == pred.shape == (R, S, 3) and not normals.requires_grad and pred.requires_grad
    assert out[FieldHeadNames.DENSITY].shape == (R, S, 1) and out[FieldHeadNames.RGB].shape == (R, S, 3)

    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ocfg = dataclasses.replace(oracle_config(cfg), predict_normals=True)
    fr = rs.frustums
    pos = (fr.origins.cpu() + fr.directions.cpu() * ((fr.starts.cpu() + fr.ends.cpu()) / 2)).reshape(-1, 3)
    q = rs.q.cpu().reshape(-1, 3)
    assert torch.equal(onf.normalized_positions(pos)[0], q)         # the oracle differentiates at the very positions the kernel is given
    ref = no.analytic(params, ocfg, q)
    relu_tie, near_face = no.ambiguous(params, ocfg, q, ref)
    keep = ~(relu_tie | near_face)
    excluded = int((~keep).sum())
    assert excluded <= no.MAX_EXCLUDED * keep.numel()
    h32 = no.density_h(params, ocfg, q, torch.float32)[0]
    with torch.no_grad():
        ref32 = {"normals": onf.field_analytic_normals(params, ocfg, pos.view(R, S, 3)).reshape(-1, 3),
                 "pred_normals": onf.field_pred_normals(params, ocfg, pos.view(R, S, 3), h32.view(R, S, -1)).reshape(-1, 3)}
    ref64 = {"normals": ref["n"], "pred_normals": no.predicted(params, ocfg, pos, ref["h"])}
    for k, got in (("normals", normals), ("pred_normals", pred)):
        got = got.detach().cpu().reshape(-1, 3)
        assert bool(torch.isfinite(got).all())
        ok, e, e_ref, limit = no.gate(got, ref64[k], ref32[k], keep)
        print(f"field {k}: e_hip {e:.2e} e_ref32 {e_ref:.2e} limit {limit:.2e} | {int(keep.sum())} compared, {excluded} excluded "
              f"({int(relu_tie.sum())} ReLU ties, {int(near_face.sum())} near a face)")
        assert ok, f"{k}: {e:.3e} > {limit:.3e}"

    # only the analytic normals: a field built without predict_normals serves them, and refuses the predicted ones
    plain, _ = make_model(small_config(precision="fp32", predict_normals=False, training_normals=True), gpu)
    only = plain.field.forward_training(rs, appearance="mean", compute_normals=True)
    assert FieldHeadNames.PRED_NORMALS not in only and torch.equal(only[FieldHeadNames.NORMALS], normals)
    with pytest.raises(ValueError, match="predict_normals"):
        plain.field.forward_training(rs, appearance="mean", compute_normals=True, pred_normals=True)
    # tiny-cuda-nn and wide fields keep raising as the training forward does
    for kw in ({"implementation": "tcnn"}, {"hidden_dim": 128, "hidden_dim_color": 128}):
        other = small_config(predict_normals=True, training_normals=True, **kw).setup().to(gpu)
        with pytest.raises(NotImplementedError):
            other.field.forward_training(rs, appearance="mean", compute_normals=True)


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def _train_batch(gpu, R=256, seed=0):
    o, d, _, _ = so.rays(R, seed=seed)
    g = torch.Generator().manual_seed(seed)
    b = RayBundle(origins=(0.4 * o).to(gpu), directions=d.to(gpu), pixel_area=torch.ones(R, 1, device=gpu),
                  camera_indices=torch.randint(0, 4, (R, 1), generator=g).to(gpu))
    return b, {"image": torch.rand(R, 3, generator=g).to(gpu)}


def _step(gpu, **kw):
    torch.manual_seed(0)
    model = _tiny_config(**kw).setup().to(gpu)
    model.train()
    b, batch = _train_batch(gpu)
    model.set_training_step(0)
    out = model(b)
    losses_ = model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch))
    sum(losses_.values()).backward()
    return model, out, losses_


def test_one_training_step_yields_the_reference_loss_dict(gpu):
    R = 256
    runs = {impl: _step(gpu, predict_normals=True, training_normals=True, training_mlp=impl) for impl in ("torch", "hip")}
    for impl, (model, out, losses_) in runs.items():
        assert set(losses_) == {"rgb_loss", "interlevel_loss", "distortion_loss", "orientation_loss", "pred_normal_loss"}, impl
        assert set(out) == BASE_KEYS | NEW_KEYS
        assert [m.implementation for m in model.modules() if isinstance(m, MLP)] == [impl] * 5    # (base, head, pred-normals, two proposal nets)
        assert out["normals"].shape == out["pred_normals"].shape == (R, 3)
        assert out["rendered_orientation_loss"].shape == out["rendered_pred_normal_loss"].shape == (R,)
        assert not out["normals"].requires_grad and not out["pred_normals"].requires_grad
        assert not out["rendered_orientation_loss"].requires_grad and out["rendered_pred_normal_loss"].requires_grad
        assert not losses_["orientation_loss"].requires_grad and losses_["pred_normal_loss"].requires_grad
        assert all(bool(torch.isfinite(out[k]).all()) for k in NEW_KEYS) and all(bool(torch.isfinite(v.detach())) for v in losses_.values())
        assert bool((out["normals"] >= 0).all()) and bool((out["normals"] <= 1).all())
        assert float(out["rendered_orientation_loss"].min()) >= 0 and float(out["rendered_orientation_loss"].max()) > 0
        cfg = model.config
        assert float(losses_["pred_normal_loss"].detach()) == pytest.approx(cfg.pred_normal_loss_mult * float(out["rendered_pred_normal_loss"].detach().mean()), rel=1e-6)
        assert float(losses_["orientation_loss"]) == pytest.approx(cfg.orientation_loss_mult * float(out["rendered_orientation_loss"].mean()), rel=1e-6)
        stacks = list(model.field.mlp_pred_normals.named_parameters()) + list(model.field.field_head_pred_normals.named_parameters())
        assert len(stacks) == 8
        for name, p in stacks:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (impl, name)
        for name, p in list(model.field.named_parameters()) + list(model.proposal_networks.named_parameters()):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (impl, name)
    # "hip" against "torch": the density gate of the MLP tests (1e-4 relative: every term here is a sum over weights) beside their rgb
    # gate (2e-5 absolute), on the loss values and on the per-ray terms before their small multipliers
    (_, out_t, loss_t), (_, out_h, loss_h) = runs["torch"], runs["hip"]
    for k in loss_t:
        t, h = float(loss_t[k].detach()), float(loss_h[k].detach())
        print(f"[training normals] {k}: torch {t:.6e} hip {h:.6e} |d| {abs(t - h):.2e}")
        assert abs(t - h) <= 1e-4 * abs(t) + 2e-5, k
    for k in ("rendered_orientation_loss", "rendered_pred_normal_loss"):
        t, h = out_t[k].detach(), out_h[k].detach()
        print(f"[training normals] {k}: largest {float(t.abs().max()):.3e}, largest difference {float((t - h).abs().max()):.2e}")
        assert bool(((t - h).abs() <= 1e-4 * t.abs() + 2e-5).all()), k


def test_with_the_flag_off_nothing_changes(gpu):
    model, out, losses_ = _step(gpu, predict_normals=True)
    assert model.config.training_normals is False
    assert set(out) == BASE_KEYS and set(losses_) == {"rgb_loss", "interlevel_loss", "distortion_loss"}
    assert all(p.grad is None for p in model.field.mlp_pred_normals.parameters())
    with pytest.raises(NotImplementedError):
        model.field.forward_training(out["ray_samples_list"][-1], compute_normals=True)
    # training_normals without predict_normals: the model's outputs are today's as well (there is no predicted normal to supervise)
    _, out2, losses2 = _step(gpu, predict_normals=False, training_normals=True)
    assert set(out2) == BASE_KEYS and set(losses2) == {"rgb_loss", "interlevel_loss", "distortion_loss"}
