"""signerf_amd/optimizers.py and signerf_amd/trainer.py, the part that needs no device: the scheduler against its closed form, the groups
``Optimizers`` builds, the state dicts of HipAdam and torch.optim.Adam in each other's ``load_state_dict``, the refusals of HipAdam, the
checkpoint's keys and the three reset flags, and tests/optim_oracle.py in fp64 against torch.optim.Adam in fp64.  No GPU."""
import math
import os

import pytest
import torch

import optim_oracle as oo
from signerf_amd import _lib
from signerf_amd.config import NerfactoModelConfig
from signerf_amd.method_config import signerf_method
from signerf_amd.optimizers import AdamOptimizerConfig, ExponentialDecaySchedulerConfig, HipAdam, Optimizers
from signerf_amd.trainer import Trainer


def _tiny_model(**kw):
    base = dict(log2_hashmap_size=10, num_proposal_samples_per_ray=(16, 8), num_nerf_samples_per_ray=8, num_train_data=4, camera_optimizer_mode="off",
                proposal_net_args_list=[{"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 128, "use_linear": False},
                                        {"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 256, "use_linear": False}])
    base.update(kw)
    return NerfactoModelConfig(**base).setup()


def _config(implementation="torch", max_norm=None):
    return {k: {"optimizer": AdamOptimizerConfig(lr=1e-2, eps=1e-15, max_norm=max_norm, implementation=implementation),
                "scheduler": ExponentialDecaySchedulerConfig(lr_final=1e-4, max_steps=1000)} for k in ("proposal_networks", "fields", "camera_opt")}


# ---- the scheduler ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ramp", ["cosine", "linear"])
def test_scheduler_values_are_the_closed_form(ramp):
    lr_init, lr_final, pre, warm, mx = 1e-2, 1e-4, 1e-8, 10, 100
    cfg = ExponentialDecaySchedulerConfig(lr_pre_warmup=pre, lr_final=lr_final, warmup_steps=warm, max_steps=mx, ramp=ramp)
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.Adam([p], lr=lr_init)
    sched = cfg.setup().get_scheduler(optimizer=opt, lr_init=lr_init)
    got = []
    for _ in range(130):
        got.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()

    def want(step):
        if step < warm:
            x = step / warm
            return pre + (lr_init - pre) * (math.sin(0.5 * math.pi * x) if ramp == "cosine" else x)
        t = min(max((step - warm) / (mx - warm), 0.0), 1.0)
        return math.exp((1 - t) * math.log(lr_init) + t * math.log(lr_final))

    for step, lr in enumerate(got):
        assert lr == pytest.approx(want(step), rel=1e-12), step
    assert got[0] == pytest.approx(pre, rel=1e-12) and got[warm] == pytest.approx(lr_init, rel=1e-12)        # step 0, the end of the warm-up
    assert got[mx] == pytest.approx(lr_final, rel=1e-12) and got[129] == pytest.approx(lr_final, rel=1e-12)   # max_steps, and beyond
    assert all(a < b for a, b in zip(got[:warm], got[1:warm + 1])) and all(a > b for a, b in zip(got[warm:mx], got[warm + 1:mx + 1]))
    if ramp == "cosine":
        assert got[5] == pytest.approx(pre + (lr_init - pre) * math.sin(math.pi / 4), rel=1e-12)
    else:
        assert got[5] == pytest.approx(pre + (lr_init - pre) * 0.5, rel=1e-12)


def test_scheduler_without_warm_up_is_the_log_lerp_over_step_by_max_steps():
    cfg = ExponentialDecaySchedulerConfig(lr_final=1e-4, max_steps=200000)
    assert (cfg.lr_pre_warmup, cfg.warmup_steps, cfg.ramp) == (1e-8, 0, "cosine")
    for step in (0, 1, 777, 100000, 200000, 250000):
        t = min(step / 200000, 1.0)
        assert cfg.lr_at(step, 1e-2) == pytest.approx(math.exp((1 - t) * math.log(1e-2) + t * math.log(1e-4)), rel=1e-14)
    assert cfg.lr_at(0, 1e-2) == pytest.approx(1e-2, rel=1e-14) and cfg.lr_at(10**7, 1e-2) == pytest.approx(1e-4, rel=1e-14)
    assert ExponentialDecaySchedulerConfig(lr_final=None, max_steps=10).lr_at(7, 3e-3) == pytest.approx(3e-3, rel=1e-14)
    with pytest.raises(ValueError, match="ramp"):
        ExponentialDecaySchedulerConfig(ramp="step").get_scheduler(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]), 1e-2)


# ---- the container ---------------------------------------------------------------------------------------------------------------------------
def test_optimizers_hands_out_the_models_groups_and_skips_an_empty_camera_opt():
    model = _tiny_model(camera_optimizer_mode="SO3xR3")
    groups = model.get_param_groups()
    assert set(groups) == {"proposal_networks", "fields", "camera_opt"} == set(signerf_method.config.optimizers)
    for impl, cls in (("torch", torch.optim.Adam), ("hip", HipAdam)):
        opts = Optimizers(_config(impl, max_norm=1.0), groups)
        assert set(opts.optimizers) == set(opts.schedulers) == set(opts.parameters) == set(groups)
        for name, params in groups.items():
            mine = [p for g in opts.optimizers[name].param_groups for p in g["params"]]
            assert type(opts.optimizers[name]) is cls and len(mine) == len([p for p in params if p.numel()]) and all(a is b for a, b in zip(mine, (p for p in params if p.numel())))
            assert opts.optimizers[name].param_groups[0]["lr"] == pytest.approx(1e-2, rel=1e-12) and opts.optimizers[name].param_groups[0]["eps"] == 1e-15
        assert opts.optimizers["fields"].defaults.get("max_norm") == (1.0 if impl == "hip" else None)
        assert opts._clips_outside("fields") == (None if impl == "hip" else 1.0)
    # the method's own registration builds, with torch's optimiser by default
    opts = Optimizers(signerf_method.config.optimizers, groups)
    assert all(type(o) is torch.optim.Adam for o in opts.optimizers.values()) and opts.optimizers["camera_opt"].param_groups[0]["lr"] == pytest.approx(1e-15, rel=1e-12)
    # camera_optimizer_mode="off": the group is absent or empty, and gets no optimiser either way
    off = _tiny_model()
    assert "camera_opt" not in off.get_param_groups()
    for groups in (off.get_param_groups(), dict(off.get_param_groups(), camera_opt=[]), dict(off.get_param_groups(), camera_opt=[torch.nn.Parameter(torch.zeros(0, 6))])):
        opts = Optimizers(_config("hip"), groups)
        assert set(opts.optimizers) == set(opts.schedulers) == {"proposal_networks", "fields"}
    with pytest.raises(RuntimeError, match="not found"):
        Optimizers({"fields": _config()["fields"]}, off.get_param_groups())
    with pytest.raises(ValueError, match="implementation"):
        AdamOptimizerConfig(implementation="cuda").setup([torch.nn.Parameter(torch.zeros(1))])


def test_the_torch_path_clips_and_steps_as_nerfstudio_does():
    """implementation="torch" on the CPU: Optimizers clips the group to max_norm, then torch.optim.Adam steps; the schedulers advance."""
    p = torch.nn.Parameter(torch.zeros(4))
    cfg = {"fields": {"optimizer": AdamOptimizerConfig(lr=1e-2, eps=1e-15, max_norm=1.0), "scheduler": ExponentialDecaySchedulerConfig(lr_final=1e-4, max_steps=10)}}
    opts = Optimizers(cfg, {"fields": [p]})
    p.grad = torch.full((4,), 3.0)
    opts.optimizer_step_all()
    assert float(torch.linalg.vector_norm(p.grad)) == pytest.approx(1.0, rel=1e-5) and float(p.detach()[0]) == pytest.approx(-1e-2, rel=1e-5)
    opts.scheduler_step_all(0)
    assert opts.optimizers["fields"].param_groups[0]["lr"] == pytest.approx(1e-2 * (1e-2) ** 0.1, rel=1e-12)
    p.grad = torch.full((4,), 3.0)
    opts.optimizer_scaler_step_all(torch.amp.GradScaler("cpu", enabled=False))
    assert float(opts.optimizers["fields"].state[p]["step"]) == 2.0
    opts.zero_grad_all()
    assert p.grad is None
    opts.optimizer_scaler_step_all(torch.amp.GradScaler("cpu", enabled=False))      # no gradient anywhere: no step
    assert float(opts.optimizers["fields"].state[p]["step"]) == 2.0


# ---- HipAdam without a device ------------------------------------------------------------------------------------------------------------
def test_state_dicts_round_trip_between_torch_adam_and_hip_adam():
    """Keys and shapes only (there is no CPU step): a torch.optim.Adam state loads into HipAdam, whose ``step`` becomes a 0-d fp32 tensor on the
    parameter's device; a HipAdam state dict loads into torch.optim.Adam, which can then step."""
    shapes = [(5, 3), (7,), (1,)]
    params = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    adam = torch.optim.Adam(params, lr=1e-2, eps=1e-15)
    for _ in range(3):
        for p in params:
            p.grad = torch.randn_like(p)
        adam.step()
    sd = adam.state_dict()
    mine = [torch.nn.Parameter(p.detach().clone()) for p in params]
    hip = HipAdam(mine, lr=5e-3, eps=1e-8, max_norm=2.0)
    assert hip._step_supports_amp_scaling is True and hip.state_dict()["state"] == {}
    hip.load_state_dict(sd)
    g = hip.param_groups[0]
    assert (g["lr"], g["eps"], g["betas"], g["weight_decay"], g["max_norm"]) == (1e-2, 1e-15, (0.9, 0.999), 0, 2.0)
    for p, q in zip(mine, params):
        st = hip.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].shape == () and st["step"].dtype == torch.float32 and st["step"].device == p.device and float(st["step"]) == 3.0
        assert torch.equal(st["exp_avg"], adam.state[q]["exp_avg"]) and torch.equal(st["exp_avg_sq"], adam.state[q]["exp_avg_sq"])
    back = hip.state_dict()
    assert set(back) == {"state", "param_groups"} and set(back["state"]) == {0, 1, 2} and set(sd["param_groups"][0]) | {"max_norm"} == set(back["param_groups"][0])
    again = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1.0)
    again.load_state_dict(back)
    assert again.param_groups[0]["lr"] == 1e-2
    for p in again.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    again.step()
    assert all(float(again.state[p]["step"]) == 4.0 and again.state[p]["exp_avg"].shape == p.shape for p in again.param_groups[0]["params"])
    # a state saved with a Python number as its step (older torch) loads too
    sd["state"][0]["step"] = 3
    hip.load_state_dict(sd)
    assert hip.state[mine[0]]["step"].shape == () and float(hip.state[mine[0]]["step"]) == 3.0
    sd["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        hip.load_state_dict(sd)


def test_hip_adam_refuses_what_it_has_no_path_for():
    p = torch.nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.ones(4, 3)
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        HipAdam([p]).step()
    for kw in ({"lr": -1.0}, {"eps": -1.0}, {"betas": (1.0, 0.999)}, {"betas": (0.9, -0.1)}, {"weight_decay": -1.0}):
        with pytest.raises(ValueError, match="Invalid"):
            HipAdam([p], **kw)
    q = torch.nn.Parameter(torch.zeros(3))      # no gradient, and an empty parameter: nothing to do, no error and no state
    opt = HipAdam([q, torch.nn.Parameter(torch.zeros(0))])
    opt.step()
    assert opt.state_dict()["state"] == {}


def test_oracle_in_fp64_is_torch_adam_in_fp64():
    """tests/optim_oracle.py against torch.optim.Adam (foreach=False) with clip_grad_norm_, both in fp64, over three steps with weight decay
    and clipping: the formulas of the header are torch's."""
    g_ = torch.Generator().manual_seed(5)
    h = oo.group(lr=1e-2, betas=(0.9, 0.999), eps=1e-15, weight_decay=0.01, max_norm=0.5)
    ps = [torch.randn(n, generator=g_, dtype=torch.float64) for n in (5, 257)]
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    adam = torch.optim.Adam(params, lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"], foreach=False)
    state = [{"p": p.clone(), "m": torch.zeros_like(p), "v": torch.zeros_like(p), "step": 0.0, "group": 0} for p in ps]
    for k in range(3):
        grads = [torch.randn(p.shape, generator=g_, dtype=torch.float64) * (10.0 if k == 1 else 0.01) for p in ps]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(params, h["max_norm"])
        adam.step()
        for t, g in zip(state, grads):
            t["g"] = g
        out, norms = oo.step(state, [h], torch.float64)
        assert float(norms[0]) == pytest.approx(float(torch.linalg.vector_norm(torch.cat(grads))), rel=1e-14)
        for t, (p, m, v, now) in zip(state, out):
            t.update(p=p, m=m, v=v, step=now)
    for t, p in zip(state, params):
        assert float((t["p"] - p.detach()).abs().max()) <= 1e-13 * float(p.detach().abs().max())
        assert float((t["m"] - adam.state[p]["exp_avg"]).abs().max()) <= 1e-13 * float(adam.state[p]["exp_avg"].abs().max())
        assert float((t["v"] - adam.state[p]["exp_avg_sq"]).abs().max()) <= 1e-13 * float(adam.state[p]["exp_avg_sq"].abs().max())
        assert t["step"] == float(adam.state[p]["step"]) == 3.0


# ---- the trainer's checkpoint ------------------------------------------------------------------------------------------------------------
def _stepped_trainer(tmp_path, **kw):
    torch.manual_seed(0)
    model = _tiny_model()
    tr = Trainer(model, None, _config("torch"), mixed_precision=True, checkpoint_dir=tmp_path, **kw)
    for p in model.parameters():
        if p.numel():
            p.grad = torch.ones_like(p)
    tr.optimizers.optimizer_step_all()
    return tr


def test_save_checkpoint_writes_the_references_four_keys(tmp_path):
    tr = _stepped_trainer(tmp_path)
    assert tr.grad_scaler.is_enabled() and tr._start_step == 0
    (tmp_path / "stale.txt").write_text("x")
    path = tr.save_checkpoint(7)
    assert path.name == "step-000000007.ckpt" and sorted(os.listdir(tmp_path)) == ["step-000000007.ckpt"]      # save_only_latest_checkpoint
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"step", "pipeline", "optimizers", "scalers"} and ck["step"] == 7
    assert set(ck["pipeline"]) == {"_model." + k for k in tr.model.state_dict()}
    assert set(ck["optimizers"]) == {"proposal_networks", "fields"} and set(ck["optimizers"]["fields"]) == {"state", "param_groups"}
    assert set(ck["scalers"]) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    tr.save_only_latest_checkpoint = False
    tr.save_checkpoint(8)
    assert sorted(os.listdir(tmp_path)) == ["step-000000007.ckpt", "step-000000008.ckpt"]
    assert Trainer(tr.model, None, _config("torch")).grad_scaler.is_enabled() is False


def test_load_checkpoint_honours_the_three_reset_flags(tmp_path):
    src = _stepped_trainer(tmp_path / "a")
    src.grad_scaler.load_state_dict(dict(src.grad_scaler.state_dict(), scale=1024.0))
    src.save_only_latest_checkpoint = False
    src.save_checkpoint(3)
    src.save_checkpoint(41)
    want = {k: v.clone() for k, v in src.model.state_dict().items()}

    def fresh(**kw):
        torch.manual_seed(1)
        return Trainer(_tiny_model(), None, _config("torch"), mixed_precision=True, **kw)

    tr = fresh()
    assert tr.load_checkpoint(tmp_path / "a").name == "step-000000041.ckpt"          # the latest one
    assert all(torch.equal(v, want[k]) for k, v in tr.model.state_dict().items()) and tr.model._weights_dirty
    opt = tr.optimizers.optimizers["fields"]
    assert len(opt.state) == len(opt.param_groups[0]["params"]) and all(float(s["step"]) == 1.0 for s in opt.state.values())
    assert tr.grad_scaler.get_scale() == 1024.0
    # the reference sets the start step to 0 whatever the flag says (signerf_trainer.py:325): restated literally
    assert tr._start_step == 0
    assert fresh().load_checkpoint(tmp_path / "a", load_step=3).name == "step-000000003.ckpt"
    with pytest.raises(FileNotFoundError):
        fresh().load_checkpoint(tmp_path / "a", load_step=4)

    tr = fresh(reset_optimizer=True)
    before = tr.optimizers
    tr.load_checkpoint(tmp_path / "a")
    assert tr.optimizers is not before and all(len(o.state) == 0 for o in tr.optimizers.optimizers.values())
    assert all(torch.equal(v, want[k]) for k, v in tr.model.state_dict().items()) and tr.grad_scaler.get_scale() == 1024.0

    tr = fresh(reset_scheduler=True)
    tr.load_checkpoint(tmp_path / "a")
    assert tr.grad_scaler.get_scale() == 65536.0 and len(tr.optimizers.optimizers["fields"].state) > 0

    tr = fresh(reset_step_count=True)
    tr.load_checkpoint(tmp_path / "a")
    assert tr._start_step == 0 and tr.grad_scaler.get_scale() == 1024.0
