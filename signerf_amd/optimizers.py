"""The optimiser side of a training step: ``HipAdam`` (torch.optim.Adam's step, gradient clipping and a GradScaler's unscale / skip in one
HIP pass, include/signerf_hip_optim.h), the two config classes the method registration names, and nerfstudio's ``Optimizers`` container
(``nerfstudio/engine/optimizers.py`` and ``schedulers.py`` of nerfstudio 1.0.2, restated: nerfstudio is not a dependency).

``HipAdam`` keeps torch.optim.Adam's state under torch's keys, so checkpoints move between the two.  It has no CPU path.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Any, Dict, Iterable, List, Optional, Tuple

import torch
from torch.optim.lr_scheduler import LambdaLR

from . import _lib

_SCALAR_KEYS = ("lr", "betas", "eps", "weight_decay", "max_norm")


def adam_step(tensors: List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, int]], groups: List[Dict[str, Any]],
              grad_scale: Optional[torch.Tensor] = None, found_inf: Optional[torch.Tensor] = None,
              workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ``sn_adam_step`` call on the current stream.  ``tensors``: (param, grad, exp_avg, exp_avg_sq, step, group index) each;
    ``groups``: dicts with lr, betas, eps, weight_decay, max_norm (None or <= 0: no clipping).  Returns the workspace (uint8), whose head
    holds one ``_lib.SnAdamRecord`` per tensor -- ``records_of`` reads them."""
    lib = _lib.load()
    T = (_lib.SnAdamTensor * max(len(tensors), 1))()
    device, total = None, 0
    for i, (p, g, m, v, step, group) in enumerate(tensors):
        for name, t in (("parameter", p), ("gradient", g), ("exp_avg", m), ("exp_avg_sq", v), ("step", step)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"HipAdam: the {name} of tensor {i} must be a torch.Tensor")
            if not t.is_cuda:
                raise _lib.SignerfHipError(f"HipAdam: the {name} of tensor {i} must live on the GPU (there is no CPU path)")
            if t.dtype != torch.float32:
                raise _lib.SignerfHipError(f"HipAdam: the {name} of tensor {i} must be fp32, not {t.dtype}")
            if not t.is_contiguous():
                raise _lib.SignerfHipError(f"HipAdam: the {name} of tensor {i} must be contiguous")
            if device is None:
                device = t.device
            elif t.device != device:
                raise _lib.SignerfHipError("HipAdam: all tensors of one step must live on one device")
        if not (g.shape == p.shape and m.shape == p.shape and v.shape == p.shape and step.numel() == 1):
            raise _lib.SignerfHipError(f"HipAdam: tensor {i}: gradient and state must have the parameter's shape, step one element")
        d = T[i]
        d.struct_size = C.sizeof(_lib.SnAdamTensor)
        d.param, d.grad, d.exp_avg, d.exp_avg_sq, d.step = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr()
        d.n, d.group = p.numel(), group
        total += p.numel()
    G = (_lib.SnAdamGroup * max(len(groups), 1))()
    for j, h in enumerate(groups):
        d = G[j]
        d.struct_size = C.sizeof(_lib.SnAdamGroup)
        d.lr, (d.beta1, d.beta2), d.eps, d.weight_decay = h["lr"], h["betas"], h["eps"], h["weight_decay"]
        d.max_norm = 0.0 if h.get("max_norm") is None else h["max_norm"]
    for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1 and t.device == (device or t.device)):
            raise _lib.SignerfHipError(f"HipAdam: {name} must be one fp32 element on the parameters' device")
    need = lib.sn_adam_workspace_bytes(len(tensors), total)
    if workspace is None or workspace.numel() < need or (device is not None and workspace.device != device):
        workspace = torch.empty(max(need, 8), dtype=torch.uint8, device=device or "cuda")
    if not tensors:
        return workspace
    with torch.cuda.device(device):
        _lib.check(lib.sn_adam_step(T, len(tensors), G, len(groups), None if grad_scale is None else grad_scale.data_ptr(),
                                    None if found_inf is None else found_inf.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                    _lib.current_stream()), None, "sn_adam_step")
    return workspace


def records_of(workspace: torch.Tensor, n_tensors: int) -> List[Dict[str, float]]:
    """The per-tensor records at the head of a workspace ``adam_step`` returned (a device-to-host copy: a diagnostic, not for the loop)."""
    raw = workspace[: n_tensors * C.sizeof(_lib.SnAdamRecord)].cpu().numpy().tobytes()
    recs = (_lib.SnAdamRecord * n_tensors).from_buffer_copy(raw)
    return [{k: getattr(r, k) for k, _ in _lib.SnAdamRecord._fields_} for r in recs]


class HipAdam(torch.optim.Optimizer):
    """torch.optim.Adam (amsgrad=False, maximize=False) whose step is one ``sn_adam_step``; ``max_norm`` adds
    ``clip_grad_norm_(params of the group, max_norm)`` to it.  Under a stock ``torch.amp.GradScaler`` the scaler's ``step`` hands over
    ``grad_scale`` / ``found_inf`` as attributes (``_step_supports_amp_scaling``) and the kernels unscale and skip: no host sync."""

    _step_supports_amp_scaling = True

    def __init__(self, params: Iterable, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_norm: Optional[float] = None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("HipAdam: lr must be a float (a tensor lr is not supported)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # the keys behind max_norm are torch.optim.Adam's, with the only values this optimiser has: a state dict of it loads into torch's
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_norm=max_norm, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self._workspace: Optional[torch.Tensor] = None

    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for k, v in self.defaults.items():      # a torch.optim.Adam group has no max_norm: the constructor's stays
                group.setdefault(k, v)
            if group["amsgrad"] or group["maximize"] or group["decoupled_weight_decay"]:
                raise ValueError("HipAdam: amsgrad, maximize and decoupled_weight_decay are not built")
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st:             # torch.optim.Adam keeps it on the host unless fused / capturable
                    st["step"] = torch.as_tensor(st["step"]).detach().to(dtype=torch.float32, device=p.device).reshape(()).clone()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        tensors, groups = [], []
        for j, group in enumerate(self.param_groups):
            groups.append({k: group[k] for k in _SCALAR_KEYS})
            for p in group["params"]:
                if p.grad is None or p.numel() == 0:
                    continue
                if p.grad.is_sparse:
                    raise _lib.SignerfHipError("HipAdam does not support sparse gradients")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                tensors.append((p, p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"], j))
        if tensors:
            scale, inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
            self._workspace = adam_step(tensors, groups, scale, inf if isinstance(inf, torch.Tensor) else None, self._workspace)
        return loss


@dataclass
class AdamOptimizerConfig:
    """nerfstudio's AdamOptimizerConfig, plus ``implementation``: "torch" builds torch.optim.Adam (``Optimizers`` clips for it, as
    nerfstudio does), "hip" builds HipAdam (which clips itself)."""

    lr: float = 1e-2
    eps: float = 1e-15
    max_norm: Optional[float] = None
    weight_decay: float = 0
    implementation: str = "torch"

    def setup(self, params) -> torch.optim.Optimizer:
        if self.implementation == "torch":
            return torch.optim.Adam(params, lr=self.lr, eps=self.eps, weight_decay=self.weight_decay)
        if self.implementation == "hip":
            return HipAdam(params, lr=self.lr, eps=self.eps, weight_decay=self.weight_decay, max_norm=self.max_norm)
        raise ValueError(f'AdamOptimizerConfig.implementation must be "torch" or "hip", not {self.implementation!r}')


@dataclass
class ExponentialDecaySchedulerConfig:
    """nerfstudio 1.0.2's ExponentialDecaySchedulerConfig.  ``lr_final`` None: the initial lr throughout."""

    lr_pre_warmup: float = 1e-8
    lr_final: Optional[float] = 1e-4
    warmup_steps: int = 0
    max_steps: int = 200000
    ramp: str = "cosine"

    def lr_at(self, step: int, lr_init: float) -> float:
        """During warm-up a ramp from lr_pre_warmup to lr_init (a quarter sine, or linear), after it
        ``exp(lerp(log lr_init, log lr_final, clip((step - warmup_steps) / (max_steps - warmup_steps), 0, 1)))`` -- with the default
        ``warmup_steps = 0`` that is ``clip(step / max_steps, 0, 1)``."""
        lr_final = lr_init if self.lr_final is None else self.lr_final
        if step < self.warmup_steps:
            x = min(max(step / self.warmup_steps, 0.0), 1.0)
            if self.ramp == "cosine":
                return self.lr_pre_warmup + (lr_init - self.lr_pre_warmup) * math.sin(0.5 * math.pi * x)
            return self.lr_pre_warmup + (lr_init - self.lr_pre_warmup) * step / self.warmup_steps
        t = min(max((step - self.warmup_steps) / (self.max_steps - self.warmup_steps), 0.0), 1.0)
        return math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)

    def get_scheduler(self, optimizer: torch.optim.Optimizer, lr_init: float) -> LambdaLR:
        if self.ramp not in ("cosine", "linear"):
            raise ValueError(f'ExponentialDecaySchedulerConfig.ramp must be "cosine" or "linear", not {self.ramp!r}')
        return LambdaLR(optimizer, lr_lambda=lambda step: self.lr_at(step, lr_init) / lr_init)   # (LambdaLR multiplies the initial lr)

    def setup(self) -> "ExponentialDecaySchedulerConfig":
        return self


class Optimizers:
    """nerfstudio's ``Optimizers``: one optimiser (and scheduler) per param group.  Groups without a parameter that has elements -- the
    ``camera_opt`` group of ``camera_optimizer_mode="off"`` -- get none."""

    def __init__(self, config: Dict[str, Dict[str, Any]], param_groups: Dict[str, List[torch.nn.Parameter]]):
        self.config = config
        self.optimizers: Dict[str, torch.optim.Optimizer] = {}
        self.schedulers: Dict[str, LambdaLR] = {}
        self.parameters: Dict[str, List[torch.nn.Parameter]] = {}
        for name, params in param_groups.items():
            params = [p for p in params if p.numel() > 0]
            if not params:
                continue
            if name not in config:
                raise RuntimeError(f'Optimizer config for "{name}" not found in the config, which names {sorted(config)}')
            lr_init = config[name]["optimizer"].lr
            self.optimizers[name] = config[name]["optimizer"].setup(params=params)
            self.parameters[name] = params
            if config[name].get("scheduler"):
                self.schedulers[name] = config[name]["scheduler"].setup().get_scheduler(optimizer=self.optimizers[name], lr_init=lr_init)

    def _clips_outside(self, name: str) -> Optional[float]:
        """the max_norm ``Optimizers`` applies itself: a HipAdam clips inside its step"""
        return None if isinstance(self.optimizers[name], HipAdam) else self.config[name]["optimizer"].max_norm

    def optimizer_step(self, param_group_name: str) -> None:
        self.optimizers[param_group_name].step()

    def scheduler_step(self, param_group_name: str) -> None:
        if param_group_name in self.schedulers:
            self.schedulers[param_group_name].step()

    def zero_grad_all(self) -> None:
        for optimizer in self.optimizers.values():
            optimizer.zero_grad()

    def optimizer_scaler_step_all(self, grad_scaler) -> None:
        for name, optimizer in self.optimizers.items():
            max_norm = self._clips_outside(name)
            if max_norm is not None:
                grad_scaler.unscale_(optimizer)
                torch.nn.utils.clip_grad_norm_(self.parameters[name], max_norm)
            if any(any(p.grad is not None for p in g["params"]) for g in optimizer.param_groups):
                grad_scaler.step(optimizer)

    def optimizer_step_all(self) -> None:
        for name, optimizer in self.optimizers.items():
            max_norm = self._clips_outside(name)
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_(self.parameters[name], max_norm)
            optimizer.step()

    def scheduler_step_all(self, step: int) -> None:
        for scheduler in self.schedulers.values():
            scheduler.step()

    def load_optimizers(self, loaded_state: Dict[str, Any]) -> None:
        for k, v in loaded_state.items():
            self.optimizers[k].load_state_dict(v)

    def load_schedulers(self, loaded_state: Dict[str, Any]) -> None:
        for k, v in loaded_state.items():
            self.schedulers[k].load_state_dict(v)
