"""The part of the reference's trainer (signerf/signerf_trainer.py, a copy of nerfstudio's ``Trainer`` with the generator hooks added) that
is not viewer or dataset generation: one training iteration over ``Optimizers``, and the checkpoint it writes and resumes from.

    trainer = Trainer(model, datamanager, signerf_method.config.optimizers, checkpoint_dir="outputs/run")
    for step in range(trainer._start_step, n):
        loss, loss_dict, metrics_dict = trainer.train_iteration(step)

The grad scaler is nerfstudio's ``GradScaler(enabled=mixed_precision)`` and is checkpointed.  ``mixed_precision=True`` together with a model
built with ``training_mlp="hip", training_mlp_precision="fp16"`` is the reference's configuration: the ``nn.Linear`` stacks then compute on
fp16 operands with fp32 accumulation (``signerf_amd.mlp``).  The scaler's factor reaches those kernels through the incoming gradient ``g``,
which they round to fp16; where the scaled ``g`` leaves fp16's range, ``r16(g)`` is inf, the inf reaches the parameter gradients, the
optimiser's found-inf path skips the step and ``update()`` halves the scale.  With the model's default ``training_mlp_precision="fp32"`` the
forward pass is fp32 and the scaler scales and unscales fp32 gradients.
"""

from __future__ import annotations

import os
from pathlib import Path
from typing import Any, Dict, Optional, Tuple

import torch

from .optimizers import Optimizers

_MODEL_PREFIX = "_model."     # a nerfstudio pipeline keeps its model under this attribute


class Trainer:
    def __init__(self, model, datamanager, optimizers_config: Dict[str, Dict[str, Any]], mixed_precision: bool = False,
                 checkpoint_dir: Optional[os.PathLike] = None, save_only_latest_checkpoint: bool = True, reset_optimizer: bool = False,
                 reset_scheduler: bool = False, reset_step_count: bool = False):
        self.model = model
        self.datamanager = datamanager
        self.optimizers_config = optimizers_config
        self.mixed_precision = mixed_precision
        self.checkpoint_dir = None if checkpoint_dir is None else Path(checkpoint_dir)
        self.save_only_latest_checkpoint = save_only_latest_checkpoint
        self.reset_optimizer, self.reset_scheduler, self.reset_step_count = reset_optimizer, reset_scheduler, reset_step_count
        self.optimizers = self.setup_optimizers()
        self.grad_scaler = torch.amp.GradScaler(model.device.type, enabled=mixed_precision)
        self._start_step = 0

    def setup_optimizers(self) -> Optimizers:
        return Optimizers(dict(self.optimizers_config), self.model.get_param_groups())

    def train_iteration(self, step: int) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
        self.optimizers.zero_grad_all()
        self.model.set_training_step(step)
        ray_bundle, batch = self.datamanager.next_train(step)
        outputs = self.model(ray_bundle)
        metrics_dict = self.model.get_metrics_dict(outputs, batch)
        loss_dict = self.model.get_loss_dict(outputs, batch, metrics_dict)
        loss = sum(loss_dict.values())
        self.grad_scaler.scale(loss).backward()
        self.optimizers.optimizer_scaler_step_all(self.grad_scaler)
        self.grad_scaler.update()
        self.optimizers.scheduler_step_all(step)
        self.model.mark_weights_dirty()     # the optimisers wrote the parameters in place: the next eval render re-uploads them
        return loss, loss_dict, metrics_dict

    def save_checkpoint(self, step: int) -> Path:
        """``step-{step:09d}.ckpt`` with the reference's four keys (signerf_trainer.py:279-306)."""
        if self.checkpoint_dir is None:
            raise ValueError("Trainer.save_checkpoint: no checkpoint_dir was given")
        self.checkpoint_dir.mkdir(parents=True, exist_ok=True)
        ckpt_path = self.checkpoint_dir / f"step-{step:09d}.ckpt"
        torch.save({"step": step,
                    "pipeline": {_MODEL_PREFIX + k: v for k, v in self.model.state_dict().items()},
                    "optimizers": {k: v.state_dict() for k, v in self.optimizers.optimizers.items()},
                    "scalers": self.grad_scaler.state_dict()}, ckpt_path)
        if self.save_only_latest_checkpoint:
            for f in self.checkpoint_dir.glob("*"):
                if f != ckpt_path:
                    f.unlink()
        return ckpt_path

    def load_checkpoint(self, load_dir: os.PathLike, load_step: Optional[int] = None) -> Path:
        """signerf_trainer.py:308-338, flag for flag."""
        load_dir = Path(load_dir)
        if load_step is None:       # the latest one (specific to the checkpoint name format)
            load_step = sorted(int(x[x.find("-") + 1: x.find(".")]) for x in os.listdir(load_dir))[-1]
        load_path = load_dir / f"step-{load_step:09d}.ckpt"
        if not load_path.exists():
            raise FileNotFoundError(f"Checkpoint {load_path} does not exist")
        loaded_state = torch.load(load_path, map_location="cpu")
        if self.reset_step_count:
            self._start_step = 0
        else:
            self._start_step = loaded_state["step"] + 1
        # The reference then sets the start step to 0 unconditionally (signerf_trainer.py:325): a SIGNeRF run resumes a nerfacto checkpoint
        # to EDIT the scene, with a fresh step count and schedule, whatever reset_step_count says.  Restated literally.
        self._start_step = 0
        self.model.load_state_dict({k[len(_MODEL_PREFIX):]: v for k, v in loaded_state["pipeline"].items() if k.startswith(_MODEL_PREFIX)})
        self.model.mark_weights_dirty()
        if self.reset_optimizer:
            self.optimizers = self.setup_optimizers()
        else:
            self.optimizers.load_optimizers(loaded_state["optimizers"])
        if not self.reset_scheduler:    # (as the reference has it: the flag governs the grad scaler's state; schedulers are not checkpointed)
            self.grad_scaler.load_state_dict(loaded_state["scalers"])
        return load_path
