"""signerf_amd/trainer.py on the GPU: the scene, sizes and gate of tests/test_gpu_sampler.py::test_a_training_loop_fits_an_analytic_scene, with
the loop run by ``Trainer.train_iteration`` over HipAdam, the scheduler, max_norm = 1 and an enabled GradScaler; then a checkpoint written and
resumed."""
import os
import sys

import pytest
import torch

from helpers import ROOT
from signerf_amd import Cameras, SIGNeRFDataManager, SIGNeRFDataManagerConfig, scene
from signerf_amd.config import NerfactoModelConfig
from signerf_amd.optimizers import AdamOptimizerConfig, ExponentialDecaySchedulerConfig, HipAdam
from signerf_amd.trainer import Trainer

pytestmark = pytest.mark.gpu


def _tiny_config():
    """tables of 2^10 rows, levels of (16, 8, 8) samples: the smallest nerfacto that still has every part (tests/test_gpu_sampler.py)"""
    return NerfactoModelConfig(log2_hashmap_size=10, num_proposal_samples_per_ray=(16, 8), num_nerf_samples_per_ray=8, num_train_data=4,
                               camera_optimizer_mode="off", training_forward=True,
                               proposal_net_args_list=[{"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 128, "use_linear": False},
                                                       {"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 256, "use_linear": False}])


def _optimizers_config():
    return {k: {"optimizer": AdamOptimizerConfig(lr=1e-2, eps=1e-15, max_norm=1.0, implementation="hip"),
                "scheduler": ExponentialDecaySchedulerConfig(lr_final=1e-4, max_steps=200000)} for k in ("proposal_networks", "fields", "camera_opt")}


def test_the_trainer_fits_an_analytic_scene_and_resumes_from_its_checkpoint(gpu, tmp_path):
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
    dm = SIGNeRFDataManager(SIGNeRFDataManagerConfig(train_num_rays_per_batch=1024), cams, images, generator=torch.Generator(device=gpu).manual_seed(0))
    model = _tiny_config().setup().to(gpu)
    model.train()
    every = torch.stack(torch.meshgrid(torch.arange(4), torch.arange(H), torch.arange(W), indexing="ij"), -1).reshape(-1, 3).to(gpu)
    all_rays, all_pixels = dm.train_ray_generator(every)

    def whole_loss():
        with torch.no_grad():
            return float(model.get_loss_dict(model(all_rays), {"image": all_pixels})["rgb_loss"])

    trainer = Trainer(model, dm, _optimizers_config(), mixed_precision=True, checkpoint_dir=tmp_path)
    assert set(trainer.optimizers.optimizers) == {"proposal_networks", "fields"} and all(type(o) is HipAdam for o in trainer.optimizers.optimizers.values())
    assert trainer.grad_scaler.is_enabled()
    first = whole_loss()
    for step in range(60):
        loss, loss_dict, metrics_dict = trainer.train_iteration(step)
    assert set(loss_dict) == {"rgb_loss", "interlevel_loss", "distortion_loss"} and "psnr" in metrics_dict and torch.isfinite(loss)
    final = whole_loss()
    steps = sorted({float(s["step"]) for o in trainer.optimizers.optimizers.values() for s in o.state.values()})
    print(f"\n[trainer fit] rgb loss {first:.5f} -> {final:.5f} ({final / first:.3f} of the initial); optimiser steps {steps}, "
          f"grad scale {trainer.grad_scaler.get_scale()}")
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert final < 0.5 * first
    lr = trainer.optimizers.optimizers["fields"].param_groups[0]["lr"]
    assert lr == pytest.approx(1e-2 * (1e-4 / 1e-2) ** (60 / 200000), rel=1e-9)          # the scheduler ran
    model.eval()
    assert torch.isfinite(model(all_rays.get_row_major_sliced_ray_bundle(0, 64))["rgb"]).all()      # the eval render after the loop
    model.train()

    # save, and load into the same trainer without resets: the next iteration runs and the field's step counters read 61
    scale = trainer.grad_scaler.get_scale()
    path = trainer.save_checkpoint(59)
    assert sorted(os.listdir(tmp_path)) == ["step-000000059.ckpt"] and set(torch.load(path, map_location="cpu")) == {"step", "pipeline", "optimizers", "scalers"}
    kept = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        for p in model.parameters():
            p.zero_()
    trainer.load_checkpoint(tmp_path)
    assert all(torch.equal(v, kept[k]) for k, v in model.state_dict().items()) and trainer.grad_scaler.get_scale() == scale
    counters = [s["step"] for o in trainer.optimizers.optimizers.values() for s in o.state.values()]
    assert counters and all(c.is_cuda and c.dtype == torch.float32 and c.shape == () for c in counters)

    def steps_of(name):
        return sorted({float(s["step"]) for s in trainer.optimizers.optimizers[name].state.values()})

    before = {k: steps_of(k) for k in trainer.optimizers.optimizers}
    loss, _, _ = trainer.train_iteration(60)
    assert torch.isfinite(loss)
    after = {k: steps_of(k) for k in trainer.optimizers.optimizers}
    print(f"[trainer resume] optimiser steps {before} -> {after}")
    # The field has a gradient in every iteration: 61 steps.  The proposal networks have one only in the iterations in which the sampler
    # updates them (every iteration up to the tenth, then ever fewer): a parameter without a gradient does not step, as in torch.
    assert before["fields"] == [60.0] and after["fields"] == [61.0]
    assert len(after["proposal_networks"]) == 1 and 10.0 <= after["proposal_networks"][0] <= 61.0
    assert after["proposal_networks"][0] - before["proposal_networks"][0] in (0.0, 1.0)
