"""``NerfactoModel`` / ``SIGNeRFModel`` -- nerfstudio-``Model``-shaped objects whose eval render runs in the HIP library.

The drop-in boundary.  What ``DatasetGenerator.render_camera`` touches
(/root/reference/signerf/datasetgenerator/datasetgenerator.py:691-701):
    graph.render_aabb, graph.eval(), graph.get_outputs_for_camera_ray_bundle(bundle) -> {"rgb","depth",...},
    graph.train(), graph.device
and what ``SIGNeRFPipeline`` touches (/root/reference/signerf/signerf_pipeline.py:93-132,151):
    model.load_state_dict(state, strict=False) with keys under ``field.``, ``proposal_networks.`` (the appearance
    embedding and camera-optimizer keys are deleted by the pipeline before the call), get_training_callbacks,
    param groups "proposal_networks" / "fields" / "camera_opt" (signerf_config.py:47-60).

The modules below hold the parameters under nerfstudio's torch-path state-dict names; their arithmetic lives in
``csrc/`` and is reached through the model's HIP handle (``signerf_amd.engine``) -- there is no PyTorch forward and no CPU fallback.
The exception is the training-side call surface of the containers themselves: ``HashEncoding.forward`` (the HIP op of
``signerf_amd.hashgrid``, differentiable), ``MLP.forward`` (its ``nn.Linear`` stack as torch ops) and ``MLPWithHashEncoding.forward``;
the eval render does not go through them.  The training forward does: ``HashMLPDensityField.get_density_training``,
``NerfactoField.forward_training`` and ``NerfactoModel.get_training_outputs`` (training-mode sampling in HIP, ``signerf_amd.samplers``;
the fields as torch ops on the modules' own parameters; compositing in HIP, ``signerf_amd.losses``).
"""

from __future__ import annotations

import re

import warnings
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import Tensor, nn

from . import _lib, mlp
from .cameras import Frustums, RaySamples, RayBundle, SceneBox  # noqa: F401
from .config import NerfactoModelConfig, SIGNeRFModelConfig
from .engine import BACKGROUNDS, INITIAL_SAMPLERS, PRECISIONS, Engine, wants_half_grid

TRAINING_MLPS = ("torch", "hip")   # config.training_mlp
TRAINING_HASHGRID_GRADS = ("atomic", "ordered")   # config.training_hashgrid_grad (hashgrid.TABLE_GRADS)
_TCNN_NORMALS = ('training_normals with implementation="tcnn": the analytic-normals kernel reads the torch-path grid and the pred-normals '
                 "stack sits behind tiny-cuda-nn's Frequency encoding; neither is built for training (config.training_tcnn trains the "
                 "fields without their normals outputs)")


# ------------------------------------------------------------------------------------------------------
# parameter containers (state-dict layout of nerfstudio's "torch" implementation)
# ------------------------------------------------------------------------------------------------------
class HashEncoding(nn.Module):
    """Parameters of nerfstudio's HashEncoding (torch path): ``hash_table`` [L*T, F].  ``trainable_tcnn``: a plain attribute
    the owning model sets under ``config.training_tcnn``; with it the forward of an ``implementation="tcnn"`` grid runs the differentiable
    tiny-cuda-nn grid (``hashgrid.hash_encode(grid="tcnn")``) instead of raising.  ``table_grad``: a plain attribute too, "atomic" or "ordered"
    (``config.training_hashgrid_grad``): how the backward pass of ``forward`` sums the table's gradient."""

    trainable_tcnn = False   # (class-level, like MLP.implementation: a module pickled whole before the attribute existed keeps refusing)
    table_grad = "atomic"    # (class-level for the same reason; not state)

    def __init__(self, num_levels: int, min_res: int, max_res: int, log2_hashmap_size: int, features_per_level: int = 2,
                 hash_init_scale: float = 0.001, implementation: str = "torch"):
        super().__init__()
        self.num_levels, self.min_res, self.max_res = num_levels, min_res, max_res
        self.log2_hashmap_size, self.features_per_level = log2_hashmap_size, features_per_level
        # "tcnn": tiny-cuda-nn grid semantics.  The table keeps the uniform [L * 2^log2_T, F] shape; a level
        # that tiny-cuda-nn indexes densely uses the first next_multiple(res^3, 8) rows of its slot (signerf_amd/tcnn_import.py).
        self.implementation = implementation
        table = torch.rand(size=((2**log2_hashmap_size) * num_levels, features_per_level)) * 2 - 1
        self.hash_table = nn.Parameter(table * hash_init_scale)

    @property
    def grid_mode(self) -> int:
        return 0 if self.implementation == "torch" else 1

    def scalings(self) -> Tensor:
        """torch: floor(min_res * growth**level), evaluated exactly as HashEncoding.__init__ does (numpy float64 growth factor
        raised to an int64 torch tensor -> fp32).  tcnn: the library's grid_scale(), exp2f(level * log2f(growth)) * base - 1."""
        growth = np.exp((np.log(self.max_res) - np.log(self.min_res)) / (self.num_levels - 1)) if self.num_levels > 1 else 1
        if self.implementation != "torch":
            log2_g = np.log2(np.float32(growth), dtype=np.float32)
            lv = np.arange(self.num_levels, dtype=np.float32)
            return torch.from_numpy(np.exp2(lv * log2_g, dtype=np.float32) * np.float32(self.min_res) - np.float32(1.0))
        levels = torch.arange(self.num_levels)
        return torch.floor(self.min_res * growth**levels).to(torch.float32)

    def get_out_dim(self) -> int:
        return self.num_levels * self.features_per_level

    def forward(self, in_tensor: Tensor) -> Tensor:
        """nerfstudio's ``HashEncoding.forward`` (torch path): positions [..., 3] in [0, 1] -> [..., L * F], differentiable in
        ``hash_table`` (and in the positions when they require a gradient) through the HIP kernels of ``signerf_amd.hashgrid``.  A
        tiny-cuda-nn grid (positions in [0, 1)) runs that module's ``grid="tcnn"`` form, when the model was built with
        ``config.training_tcnn``."""
        if self.implementation != "torch" and not self.trainable_tcnn:
            raise NotImplementedError(f'HashEncoding.forward: implementation={self.implementation!r}: only the torch-path grid is trainable '
                                      "here; the tiny-cuda-nn grid (its own resolutions, dense coarse levels) trains behind "
                                      "config.training_tcnn=True")
        from . import hashgrid

        dev = in_tensor.device if isinstance(in_tensor, Tensor) else None
        return hashgrid.hash_encode(in_tensor, self.hash_table, self._scalings_on(dev), self.log2_hashmap_size,
                                    grid="torch" if self.implementation == "torch" else "tcnn", table_grad=self.table_grad)

    def _scalings_on(self, dev) -> Tensor:
        """The scalings are a function of the constructor's arguments: cached per device, NOT a buffer (the state dict stays hash_table only)."""
        cache = self.__dict__.setdefault("_scalings_cache", {})
        if dev not in cache:
            cache[dev] = self.scalings().to(dev)
        return cache[dev]


class MLP(nn.Module):
    """Parameters of nerfstudio's torch MLP: ``layers`` = nn.Linear list (A8).  ``implementation``: "torch" -- ``forward`` is the torch ops
    below -- or "hip": the same parameters through ``mlp.fused_mlp`` (one HIP kernel per pass; GPU tensors, at most 4 layers of at most 64
    units).  ``precision``: "fp32", or "fp16" -- the fused op's mixed precision (fp16 operands, fp32 accumulation, these fp32 parameters as
    the master copy), which exists for "hip" alone.  Plain attributes, not state: the state dict is the same either way."""

    implementation = "torch"   # (class-level: a module pickled whole before the attribute existed still runs the torch ops)
    precision = "fp32"         # (class-level, for the same reason)

    def __init__(self, in_dim: int, num_layers: int, layer_width: int, out_dim: int, implementation: str = "torch"):
        super().__init__()
        dims = [in_dim] + [layer_width] * (num_layers - 1) + [out_dim]
        self.layers = nn.ModuleList([nn.Linear(dims[i], dims[i + 1]) for i in range(num_layers)])
        self.implementation = implementation

    def forward(self, in_tensor: Tensor) -> Tensor:
        """The ``nn.Linear`` stack with a ReLU between layers and no output activation (torch ops; ``oracle.nerfacto.mlp_forward``)."""
        if self.implementation == "hip":
            return mlp.fused_mlp(in_tensor, [layer.weight for layer in self.layers], [layer.bias for layer in self.layers], self.precision)
        if self.implementation != "torch":
            raise ValueError(f'MLP.implementation={self.implementation!r}: "torch" or "hip" expected')
        if self.precision != "fp32":
            raise ValueError(f'MLP.precision={self.precision!r} with implementation="torch": the torch path is fp32 here; the mixed-precision '
                             'arithmetic is the fused HIP op\'s and needs implementation="hip"')
        x = in_tensor
        for i, layer in enumerate(self.layers):
            x = layer(x)
            if i < len(self.layers) - 1:
                x = torch.relu(x)
        return x


class MLPWithHashEncoding(nn.Module):
    def __init__(self, num_levels, min_res, max_res, log2_hashmap_size, features_per_level, num_layers, layer_width, out_dim,
                 implementation: str = "torch"):
        super().__init__()
        self.encoder = HashEncoding(num_levels, min_res, max_res, log2_hashmap_size, features_per_level, implementation=implementation)
        self.mlp = MLP(num_levels * features_per_level, num_layers, layer_width, out_dim)

    def forward(self, in_tensor: Tensor) -> Tensor:
        return self.mlp(self.encoder(in_tensor))


class Embedding(nn.Module):
    def __init__(self, in_dim: int, out_dim: int):
        super().__init__()
        self.embedding = nn.Embedding(in_dim, out_dim)

    def mean(self, dim=0):
        return self.embedding.weight.mean(dim)


class PredNormalsFieldHead(nn.Module):
    """Parameters of nerfstudio's PredNormalsFieldHead: ``net`` = Linear(in_dim, 3) (followed by tanh and L2 normalisation)."""

    def __init__(self, in_dim: int):
        super().__init__()
        self.net = nn.Linear(in_dim, 3)


class CameraOptimizer(nn.Module):
    """Parameters of nerfstudio's ``CameraOptimizer`` [NS]: ``pose_adjustment`` [num_cameras, 6] (so3 + translation), zeros at
    init.  It adjusts TRAINING rays only (``apply_to_raybundle`` is a no-op in eval mode), so the render path never reads it; it
    exists so that the "camera_opt" param group of signerf_config.py:56-59 and the ``camera_optimizer.*`` state-dict keys
    (deleted by signerf_pipeline.py:110-131 before loading, kept by plain nerfacto checkpoints) have their counterpart."""

    def __init__(self, num_cameras: int, mode: str = "SO3xR3"):
        super().__init__()
        self.mode = mode
        if mode != "off":
            self.pose_adjustment = nn.Parameter(torch.zeros((num_cameras, 6)))

    def get_param_groups(self, param_groups: dict) -> None:
        params = list(self.parameters())
        if self.mode != "off":
            assert len(params) > 0
            param_groups["camera_opt"] = params


try:  # inside a nerfstudio installation the Field outputs are keyed by ITS enum (members of different Enum classes never compare equal)
    from nerfstudio.field_components.field_heads import FieldHeadNames  # type: ignore  # noqa: F401
except Exception:  # pragma: no cover  (nerfstudio is not installed in the build container)
    import enum

    class FieldHeadNames(enum.Enum):
        """nerfstudio's ``FieldHeadNames`` values [NS-RECALL, H] -- the keys of ``Field.forward`` / ``get_outputs``."""

        RGB = "rgb"
        SH = "sh"
        DENSITY = "density"
        NORMALS = "normals"
        PRED_NORMALS = "pred_normals"
        UNCERTAINTY = "uncertainty"
        BACKGROUND_RGB = "background_rgb"
        TRANSIENT_RGB = "transient_rgb"
        TRANSIENT_DENSITY = "transient_density"
        SEMANTICS = "semantics"
        SDF = "sdf"
        ALPHA = "alpha"
        GRADIENT = "gradient"


class _HipField(nn.Module):
    """nerfstudio's ``Field`` call surface [NS-RECALL, H] as thin bindings over the stage entry point ``sn_field_forward_geo`` (the LITERAL
    torch-path arithmetic, eval mode).  signerf/signerf.py:27 subclasses NerfactoModel and so inherits ``model.field`` /
    ``model.proposal_networks[i]`` with these methods; nerfstudio's samplers (``density_fns``) and export tools call them.

        density_fn(positions [...,3])                 -> density [...,1]
        get_density(ray_samples)                      -> (density [...,1], base_mlp_out [...,15] | None)
        get_outputs(ray_samples, density_embedding)   -> {FieldHeadNames.RGB: [...,3]}                      (main field)
        forward(ray_samples, compute_normals=False)   -> {FieldHeadNames.DENSITY: ..., FieldHeadNames.RGB: ...}

    The parameters live in the owning model's HIP handle, so a Field evaluates through its owner (set by ``populate_modules``); there
    is no PyTorch forward and no CPU path."""

    _which = -1  # -1: the main field; i >= 0: proposal network i

    def _bind(self, owner, which: int) -> None:
        import weakref

        object.__setattr__(self, "_owner_ref", weakref.ref(owner))   # not a sub-module: no reference cycle, not in the state dict
        object.__setattr__(self, "_which", which)

    def _owner(self):
        owner = getattr(self, "_owner_ref", lambda: None)()
        if owner is None:
            raise _lib.SignerfHipError("this Field is not attached to a model: its parameters are evaluated through the owning "
                                       "NerfactoModel's HIP handle (there is no PyTorch forward)")
        return owner

    @torch.no_grad()
    def _evaluate(self, positions: Tensor, directions: Optional[Tensor], want_geo: bool):
        from . import ops

        owner = self._owner()
        if positions.shape[-1] != 3:
            raise ValueError("positions must be [..., 3]")
        shape = positions.shape[:-1]
        dev = owner.device
        pos = positions.reshape(-1, 3).to(device=dev, dtype=torch.float32)
        d = None if directions is None else directions.reshape(-1, 3).to(device=dev, dtype=torch.float32)
        if pos.shape[0] == 0:
            z = lambda c: torch.empty((*shape, c), dtype=torch.float32, device=dev)  # noqa: E731
            return z(1), (None if d is None or self._which >= 0 else z(3)), (z(15) if want_geo else None)
        if want_geo:
            density, rgb, geo = ops.field_forward(owner, pos, d, self._which, return_geo=True)
        else:
            (density, rgb), geo = ops.field_forward(owner, pos, d, self._which), None
        return (density.view(*shape, 1), None if rgb is None else rgb.view(*shape, 3), None if geo is None else geo.view(*shape, 15))

    def density_fn(self, positions: Tensor, times: Optional[Tensor] = None) -> Tensor:
        """``Field.density_fn``: density at world positions (the scene contraction / normalisation is part of the field)."""
        return self._evaluate(positions, None, False)[0]

    def get_density(self, ray_samples):
        positions = ray_samples.frustums.get_positions()
        density, _, geo = self._evaluate(positions, None, self._which < 0)
        return density, geo

    def forward(self, ray_samples, compute_normals: bool = False) -> Dict:
        if compute_normals:
            raise NotImplementedError("per-sample normals are not exposed: the composited 'normals' / 'pred_normals' outputs of the model "
                                      "are (NerfactoModel.get_outputs_for_camera_ray_bundle, csrc/sn_normals.h)")
        fr = ray_samples.frustums
        density, rgb, _ = self._evaluate(fr.get_positions(), fr.directions if self._which < 0 else None, False)
        out = {FieldHeadNames.DENSITY: density}
        if rgb is not None:
            out[FieldHeadNames.RGB] = rgb
        return out


class _TruncExp(torch.autograd.Function):
    """nerfstudio's ``trunc_exp`` [NS-RECALL, field_components/activations.py]: exp forwards, exp(clamp(x, max=15)) backwards."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, max=15.0))


_SH4 = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.9461746957575601, 0.31539156525251999, 0.5462742152960396,
        0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 1.445305721320277)


def _sh4_encoding(directions: Tensor, remap: str = "torch") -> Tensor:
    """The 16 real SH components of degree < 4 in the eval kernel's conventions: for the torch path evaluated on
    ``get_normalized_directions`` = (d + 1) / 2, for ``remap="tcnn"`` on that value mapped back to [-1, 1], as
    tiny-cuda-nn does (``oracle.nerfacto.direction_encoding``).  [..., 3] -> [..., 16]."""
    d = (directions + 1.0) / 2.0
    if remap != "torch":
        d = d * 2.0 - 1.0
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz = x * x, y * y, z * z
    c0, c1, c2, c3, c4, c5, c6, c7, c8, c9, c10 = _SH4
    return torch.stack([torch.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * zz - c4, c2 * x * z, c5 * (xx - yy),
                        c6 * y * (3 * xx - yy), c7 * x * y * z, c8 * y * (5 * zz - 1), c9 * z * (5 * zz - 3), c8 * x * (5 * zz - 1),
                        c10 * z * (xx - yy), c6 * x * (xx - 3 * yy)], dim=-1)


def _training_q(owner, ray_samples):
    """The field's normalised positions of training samples, already multiplied by the selector, and the selector [..., 1] (fp32).
    Samples of ``signerf_amd.samplers`` carry both (the sampler kernels' ``q`` / ``selector``, the contraction case); with
    ``disable_scene_contraction`` -- or samples from elsewhere -- they are torch ops on the frustums' positions."""
    cfg = owner.config
    if cfg.implementation != "torch" and not cfg.training_tcnn:
        raise NotImplementedError(f"training forward: implementation={cfg.implementation!r}: only the torch-path fields train here (the "
                                  "tiny-cuda-nn grid trains behind config.training_tcnn=True)")
    if cfg.hidden_dim != 64 or cfg.hidden_dim_color != 64:
        raise NotImplementedError("training forward: wide fields (hidden_dim=128) are not built for training")
    q, sel = getattr(ray_samples, "q", None), getattr(ray_samples, "selector", None)
    if cfg.disable_scene_contraction or q is None or sel is None:
        pos = ray_samples.frustums.get_positions()
        if cfg.disable_scene_contraction:
            aabb = (owner.scene_box.aabb if owner.scene_box is not None else torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])).to(pos)
            q = (pos - aabb[0]) / (aabb[1] - aabb[0])
        else:
            mag = torch.linalg.norm(pos, ord=float("inf"), dim=-1)[..., None]
            q = (torch.where(mag < 1, pos, (2 - (1 / mag)) * (pos / mag)) + 2.0) / 4.0
        sel = ((q > 0.0) & (q < 1.0)).all(dim=-1)
        q = q * sel[..., None]
    return q.detach(), sel[..., None].to(torch.float32)


class NerfactoField(_HipField):
    """Parameters of nerfstudio's NerfactoField (A6-A9, A13-A15) + its eval-mode call surface (``_HipField``)."""

    def __init__(self, config: NerfactoModelConfig, num_images: int):
        super().__init__()
        self.geo_feat_dim = 15
        self.mlp_base = MLPWithHashEncoding(config.num_levels, config.base_res, config.max_res, config.log2_hashmap_size,
                                            config.features_per_level, 2, config.hidden_dim, 1 + self.geo_feat_dim,
                                            implementation=config.implementation)
        self.embedding_appearance = Embedding(num_images, config.appearance_embed_dim)
        self.mlp_head = MLP(16 + self.geo_feat_dim + config.appearance_embed_dim, 3, config.hidden_dim_color, 3)
        if config.predict_normals:  # row a16: NeRFEncoding(2 frequencies) of the position (12) + geo features -> 64 -> 64 -> 64 -> head
            self.mlp_pred_normals = MLP(12 + self.geo_feat_dim, 3, 64, 64)
            self.field_head_pred_normals = PredNormalsFieldHead(64)

    def get_outputs(self, ray_samples, density_embedding: Optional[Tensor] = None) -> Dict:
        """``NerfactoField.get_outputs``: {RGB: [...,3]} for the samples' positions and directions, eval mode (mean appearance embedding, A14).
        ``density_embedding`` is a function of the positions; the kernel evaluates the whole field from them in one pass, so the
        argument is only checked for its shape (``Field.forward`` always passes the value ``get_density`` returned for the same samples)."""
        fr = ray_samples.frustums
        if density_embedding is not None and tuple(density_embedding.shape) != (*fr.directions.shape[:-1], self.geo_feat_dim):
            raise ValueError(f"density_embedding must be [..., {self.geo_feat_dim}] for these samples")
        _, rgb, _ = self._evaluate(fr.get_positions(), fr.directions, False)
        return {FieldHeadNames.RGB: rgb}

    def forward_training(self, ray_samples, appearance: str = "per_camera", compute_normals: bool = False, return_geo: bool = False,
                         pred_normals: Optional[bool] = None) -> Dict:
        """The field as DIFFERENTIABLE torch ops on this module's own parameters, around the HIP hash grid (``mlp_base`` =
        ``HashEncoding.forward`` + the ``nn.Linear`` stack): {DENSITY: [...,1], RGB: [...,3]}.  The arithmetic is the eval field's
        (``oracle.nerfacto.density_field`` / ``field_rgb``): density = average_init_density trunc_exp(h_0) selector, the SH-4 direction
        encoding on (d + 1) / 2, ``mlp_head`` and a sigmoid.  ``appearance``: "per_camera" -- the embedding row of every sample's
        ``camera_indices``, what nerfstudio does while training -- or "mean", the table's mean (eval with the average embedding).  The HIP
        handle is not involved: after an optimizer step ``mark_weights_dirty()`` is still needed before the next eval render.
        ``compute_normals`` (``config.training_normals`` only; otherwise ``NotImplementedError``) adds NORMALS [...,3], the analytic
        normals on the same masked ``q`` the base stack sees -- HIP, no gradient, on any field -- and PRED_NORMALS [...,3], differentiable
        in the pred-normals stack, its head and the geo features: on a ``predict_normals`` field by default, or as ``pred_normals`` says
        (True on a field built without ``predict_normals`` raises ``ValueError``)."""
        owner = self._owner()
        cfg = owner.config
        if compute_normals and not cfg.training_normals:
            raise NotImplementedError("forward_training: per-sample normals (analytic or predicted) are built for training behind "
                                      "config.training_normals=True; without it a predict_normals=True model trains without its normals "
                                      "outputs")
        if compute_normals and cfg.implementation != "torch":
            raise NotImplementedError(_TCNN_NORMALS)
        if appearance not in ("per_camera", "mean"):
            raise ValueError(f'appearance={appearance!r}: "per_camera" or "mean" expected')
        q, sel = _training_q(owner, ray_samples)
        lead = q.shape[:-1]
        h = self.mlp_base(q.reshape(-1, 3))
        density = (cfg.average_init_density * _TruncExp.apply(h[:, :1])).reshape(*lead, 1) * sel
        geo = h[:, 1:1 + self.geo_feat_dim]
        parts = [_sh4_encoding(ray_samples.frustums.directions.reshape(-1, 3), "torch" if cfg.implementation == "torch" else "tcnn"), geo]
        if cfg.appearance_embed_dim > 0:
            if appearance == "per_camera":
                if ray_samples.camera_indices is None:
                    raise ValueError('forward_training(appearance="per_camera"): the ray samples carry no camera_indices')
                app = self.embedding_appearance.embedding(ray_samples.camera_indices.reshape(-1).long())
            else:
                app = self.embedding_appearance.mean(0)[None, :].expand(h.shape[0], -1)
            parts.append(app)
        rgb = torch.sigmoid(self.mlp_head(torch.cat(parts, dim=-1))).reshape(*lead, 3)
        out = {FieldHeadNames.DENSITY: density, FieldHeadNames.RGB: rgb}
        if return_geo:
            out["geo"] = geo.reshape(*lead, self.geo_feat_dim)
        if compute_normals:
            out[FieldHeadNames.NORMALS] = self._training_analytic_normals(q)
            if cfg.predict_normals if pred_normals is None else pred_normals:
                out[FieldHeadNames.PRED_NORMALS] = self._training_pred_normals(ray_samples, geo).reshape(*lead, 3)
        return out

    def _training_analytic_normals(self, q: Tensor) -> Tensor:
        """``Field.get_normals`` of training samples, [..., 3], on the masked positions ``q`` the base stack sees: minus the normalised
        gradient of the pre-activation density in ``q``, by the fused HIP kernel of ``signerf_amd.train_normals`` (measured faster than the
        two-launch route on this shape: DESIGN.md §4 "Training-mode normals").  A constant for autograd, as in nerfstudio
        (``torch.autograd.grad`` without ``create_graph``)."""
        from . import train_normals

        enc, layers = self.mlp_base.encoder, self.mlp_base.mlp.layers
        return train_normals.analytic_normals(q, enc.hash_table, enc._scalings_on(q.device), enc.log2_hashmap_size,
                                              [layer.weight for layer in layers], [layer.bias for layer in layers])

    def _training_pred_normals(self, ray_samples, geo: Tensor) -> Tensor:
        """The pred-normal branch of ``NerfactoField.get_outputs`` (``oracle.nerfacto.field_pred_normals``, torch path):
        cat[NeRFEncoding(2 frequencies) of the WORLD positions (12), geo (15)] -> ``mlp_pred_normals`` -> Linear(64, 3) -> tanh ->
        ``F.normalize``, [N, 3].  Differentiable in the stack, the head and ``geo``; the positions get no gradient."""
        if not hasattr(self, "mlp_pred_normals"):
            raise ValueError("forward_training: PRED_NORMALS asked of a field built without predict_normals")
        pos = ray_samples.frustums.get_positions().detach().reshape(-1, 3)
        scaled = 2.0 * np.pi * pos
        si = (scaled[..., None] * torch.tensor([1.0, 2.0], dtype=pos.dtype, device=pos.device)).reshape(pos.shape[0], -1)
        enc = torch.sin(torch.cat([si, si + np.pi / 2.0], dim=-1))
        x = self.mlp_pred_normals(torch.cat([enc, geo], dim=-1))
        return torch.nn.functional.normalize(torch.tanh(self.field_head_pred_normals.net(x)), dim=-1)


class HashMLPDensityField(_HipField):
    """Parameters of a proposal network (row a9) + ``density_fn`` / ``get_density`` (``_HipField``; ``get_density`` returns
    ``(density, None)`` as nerfstudio's does)."""

    def __init__(self, hidden_dim=16, log2_hashmap_size=17, num_levels=5, max_res=128, base_res=16, features_per_level=2,
                 use_linear=False, implementation="torch", **_):
        super().__init__()
        if use_linear:
            raise NotImplementedError("use_linear proposal nets (a Linear layer instead of the hash grid + MLP) are not supported: nerfacto's and "
                                      "SIGNeRF's proposal_net_args_list set use_linear=False")
        self.mlp_base = MLPWithHashEncoding(num_levels, base_res, max_res, log2_hashmap_size, features_per_level, 2, hidden_dim, 1,
                                            implementation=implementation)

    def get_density_training(self, ray_samples) -> Tensor:
        """The proposal network as DIFFERENTIABLE torch ops on this module's own parameters, around the HIP hash grid: density [...,1] =
        average_init_density trunc_exp(mlp_base(q)) selector (``oracle.nerfacto.density_field``).  What a training-mode
        ``ProposalNetworkSampler`` is handed as its density function."""
        owner = self._owner()
        q, sel = _training_q(owner, ray_samples)
        h = self.mlp_base(q.reshape(-1, 3))
        return (owner.config.average_init_density * _TruncExp.apply(h)).reshape(*q.shape[:-1], 1) * sel


class LazyOutputs(dict):
    """The outputs dict of a render whose "normals" / "pred_normals" entries (row a16) are rendered on first use: reading either
    key, or enumerating the dict (keys / items / values / iteration / len / ``in``), launches the normals kernel once."""

    _PENDING = ("normals", "pred_normals")

    def __init__(self, base: Dict[str, Tensor], producer):
        super().__init__(base)
        self._producer = producer

    def _materialise(self):
        if self._producer is not None:
            producer, self._producer = self._producer, None
            super().update(producer())

    def __missing__(self, key):
        if key in self._PENDING and self._producer is not None:
            self._materialise()
            return super().__getitem__(key)
        raise KeyError(key)

    def get(self, key, default=None):
        if key in self._PENDING:
            self._materialise()
        return super().get(key, default)

    def __contains__(self, key):
        return super().__contains__(key) or (key in self._PENDING and self._producer is not None)

    def keys(self):
        self._materialise()
        return super().keys()

    def items(self):
        self._materialise()
        return super().items()

    def values(self):
        self._materialise()
        return super().values()

    def __iter__(self):
        self._materialise()
        return super().__iter__()

    def __len__(self):
        self._materialise()
        return super().__len__()

    def copy(self):
        self._materialise()
        return dict(self)


# ------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------
def _desc_of(enc: HashEncoding, hidden_dim: int, out_dim: int) -> _lib.SnHashMlpDesc:
    d = _lib.SnHashMlpDesc()
    d.num_levels = enc.num_levels
    d.features_per_level = enc.features_per_level
    d.log2_hashmap_size = enc.log2_hashmap_size
    d.hidden_dim = hidden_dim
    d.num_layers = 2
    d.out_dim = out_dim
    d.grid_mode = enc.grid_mode
    sc = enc.scalings().tolist()
    for i in range(_lib.SN_MAX_LEVELS):
        d.scalings[i] = sc[i] if i < len(sc) else 0.0
    return d


def _median_depth(weights: Tensor, ray_samples) -> Tensor:
    """``DepthRenderer("median")`` (``oracle.nerfacto.render_depth_median``) as torch ops: weights [R,S,1] -> [R,1]."""
    steps = (ray_samples.frustums.starts + ray_samples.frustums.ends) / 2
    cumulative = torch.cumsum(weights[..., 0], dim=-1)
    split = torch.full((*weights.shape[:-2], 1), 0.5, dtype=weights.dtype, device=weights.device)
    idx = torch.clamp(torch.searchsorted(cumulative.contiguous(), split, side="left"), 0, steps.shape[-2] - 1)
    return torch.gather(steps[..., 0], dim=-1, index=idx)


def _expected_depth(weights: Tensor, ray_samples) -> Tensor:
    """``DepthRenderer("expected")`` (``oracle.nerfacto.render_depth_expected``) as torch ops; the clip bounds span the bundle."""
    steps = (ray_samples.frustums.starts + ray_samples.frustums.ends) / 2
    depth = torch.sum(weights * steps, dim=-2) / (torch.sum(weights, -2) + 1e-10)
    return torch.clip(depth, steps.min(), steps.max()) if steps.numel() else depth


class NerfactoModel(nn.Module):
    """Eval-mode nerfacto render on MI355X behind nerfstudio's ``Model`` surface."""

    config: NerfactoModelConfig

    def __init__(self, config: NerfactoModelConfig, scene_box: Optional[SceneBox] = None, num_train_data: Optional[int] = None,
                 **kwargs):
        super().__init__()
        self.config = config
        self.scene_box = scene_box
        self.render_aabb: Optional[SceneBox] = None  # datasetgenerator.py:691 reads this
        self.num_train_data = num_train_data if num_train_data is not None else config.num_train_data
        self.kwargs = kwargs
        self.device_indicator_param = nn.Parameter(torch.empty(0))
        self._engine = Engine(self)   # the eval-mode HIP handle: a plain object that holds the model weakly (signerf_amd.engine)
        self.populate_modules()

    # -- module set-up (names = nerfstudio's; signerf.py:32-39 overrides this and calls super) -------------
    def populate_modules(self):
        cfg = self.config
        # the kernels implement the values SIGNeRF runs with (nerfacto's defaults); anything else must not render silently wrong
        if cfg.background_color not in BACKGROUNDS:
            raise NotImplementedError(f"background_color={cfg.background_color!r}: one of {sorted(BACKGROUNDS)} expected")
        if cfg.precision not in PRECISIONS:
            raise NotImplementedError(f"precision={cfg.precision!r}: one of {sorted(PRECISIONS)} expected")
        if cfg.precision == "fp16" and cfg.implementation != "tcnn":
            raise NotImplementedError('precision="fp16" (single fp16 operands, fp16 activations between layers) is the arithmetic of '
                                      'tiny-cuda-nn checkpoints: it needs implementation="tcnn"; the torch-path parity target runs "fp16x2" / "fp32"')
        if cfg.proposal_initial_sampler not in INITIAL_SAMPLERS:
            raise NotImplementedError(f"proposal_initial_sampler={cfg.proposal_initial_sampler!r}: one of {sorted(INITIAL_SAMPLERS)} expected")
        # a wide field (hidden_dim = hidden_dim_color = 128, nerfacto-big) has no normals kernel: the lazy "normals" / "pred_normals" surface
        # the library's refusal when they are read, but "always" would make every render fail
        if cfg.hidden_dim == 128 and cfg.predict_normals and cfg.compute_normals == "always":
            raise NotImplementedError('compute_normals="always" with a wide field (hidden_dim=128): the normals kernel is not built for wide '
                                      'fields; use compute_normals="lazy" (rgb / depth render, reading the normals raises) or "never"')
        self.field = NerfactoField(cfg, self.num_train_data)
        self.proposal_networks = nn.ModuleList()
        for i in range(cfg.num_proposal_iterations):
            args = cfg.proposal_net_args_list[min(i, len(cfg.proposal_net_args_list) - 1)]
            self.proposal_networks.append(HashMLPDensityField(**args, implementation=cfg.implementation))
        self.field._bind(self, -1)
        for i, net in enumerate(self.proposal_networks):
            net._bind(self, i)
        self.density_fns = [net.density_fn for net in self.proposal_networks]   # nerfstudio's NerfactoModel attribute [NS-RECALL, H]
        if cfg.training_mlp not in TRAINING_MLPS:
            raise ValueError(f"training_mlp={cfg.training_mlp!r}: one of {sorted(TRAINING_MLPS)} expected")
        mlp.check_precision(cfg.training_mlp_precision)
        if cfg.training_mlp_precision != "fp32" and cfg.training_mlp != "hip":
            raise NotImplementedError(f'training_mlp_precision={cfg.training_mlp_precision!r} with training_mlp={cfg.training_mlp!r}: the '
                                      'mixed-precision arithmetic is the fused HIP MLP\'s; it needs training_mlp="hip" (the torch stacks are fp32)')
        if cfg.training_hashgrid_grad not in TRAINING_HASHGRID_GRADS:
            raise ValueError(f"training_hashgrid_grad={cfg.training_hashgrid_grad!r}: one of {sorted(TRAINING_HASHGRID_GRADS)} expected")
        if cfg.training_hashgrid_grad != "atomic":
            for net in [self.field.mlp_base] + [net.mlp_base for net in self.proposal_networks]:
                net.encoder.table_grad = cfg.training_hashgrid_grad
        if cfg.implementation != "torch" and cfg.training_tcnn:
            if cfg.training_normals:
                raise NotImplementedError(_TCNN_NORMALS)
            for m in self.modules():
                if isinstance(m, HashEncoding):
                    m.trainable_tcnn = True
        if cfg.training_mlp == "hip":
            if cfg.implementation != "torch" and not cfg.training_tcnn:
                raise NotImplementedError(f'training_mlp="hip" with implementation={cfg.implementation!r}: the HIP MLP reads the nn.Linear '
                                          "weights of the torch-path fields; a tiny-cuda-nn field trains behind config.training_tcnn=True")
            stacks = [self.field.mlp_base.mlp, self.field.mlp_head] + [net.mlp_base.mlp for net in self.proposal_networks]
            if cfg.predict_normals:
                stacks.append(self.field.mlp_pred_normals)
            for stack in stacks:
                try:
                    mlp.check_dims([stack.layers[0].in_features] + [layer.out_features for layer in stack.layers])
                except ValueError as e:
                    raise NotImplementedError(f'training_mlp="hip": {e}; wide fields train with training_mlp="torch"') from None
                stack.implementation, stack.precision = "hip", cfg.training_mlp_precision
        self.camera_optimizer = CameraOptimizer(self.num_train_data, cfg.camera_optimizer_mode)

    @property
    def device(self):
        return self.device_indicator_param.device

    @property
    def _has_pred_normals(self) -> bool:
        """``predict_normals=True`` (signerf_config.py:33) gives the field its pred-normal MLP, in both implementations (a tiny-cuda-nn
        checkpoint's flat vector is unpacked by tcnn_import)."""
        return self.config.predict_normals

    # -- plugin surface the pipeline / trainer expect ---------------------------------------------------------
    def get_param_groups(self) -> Dict[str, List[nn.Parameter]]:
        """nerfstudio's NerfactoModel.get_param_groups [NS]: the three groups signerf_config.py:47-60 attaches optimizers to."""
        groups = {"proposal_networks": list(self.proposal_networks.parameters()), "fields": list(self.field.parameters())}
        self.camera_optimizer.get_param_groups(param_groups=groups)
        return groups

    def get_training_callbacks(self, training_callback_attributes=None) -> List:
        return []

    def _gt_rgb(self, batch) -> Tensor:
        image = batch["image"].to(self.device)
        if image.shape[-1] != 3:
            raise NotImplementedError(f"batch['image'] with {image.shape[-1]} channels: the losses take RGB images (alpha blending of the "
                                      "ground truth is not built)")
        return image

    def get_metrics_dict(self, outputs, batch) -> dict:
        """nerfstudio's NerfactoModel.get_metrics_dict [NS-RECALL]: ``psnr`` (data range 1), and while training ``distortion``, the mean
        distortion loss of the main level (losses.distortion_loss, HIP) when the outputs hold ``weights_list``."""
        from . import losses

        mse = torch.mean((outputs["rgb"] - self._gt_rgb(batch)) ** 2)
        metrics = {"psnr": -10.0 * torch.log10(mse)}
        if self.training and "weights_list" in outputs:
            metrics["distortion"] = losses.distortion_loss(outputs["weights_list"], outputs["ray_samples_list"])
        return metrics

    def _sampler_losses(self, outputs, metrics_dict) -> dict:
        """The training-only terms nerfacto and SIGNeRF share: interlevel and distortion loss with the config's multipliers, and the two
        normal losses when the outputs hold their per-ray terms (``get_training_outputs`` of a ``predict_normals`` model under
        ``config.training_normals``; an eval render never does)."""
        from . import losses

        cfg = self.config
        out = {"interlevel_loss": cfg.interlevel_loss_mult * losses.interlevel_loss(outputs["weights_list"], outputs["ray_samples_list"])}
        if metrics_dict is not None and "distortion" in metrics_dict:
            distortion = metrics_dict["distortion"]
        else:
            distortion = losses.distortion_loss(outputs["weights_list"], outputs["ray_samples_list"])
        out["distortion_loss"] = cfg.distortion_loss_mult * distortion
        if cfg.predict_normals:
            if "rendered_orientation_loss" in outputs:
                out["orientation_loss"] = cfg.orientation_loss_mult * torch.mean(outputs["rendered_orientation_loss"])
            if "rendered_pred_normal_loss" in outputs:
                out["pred_normal_loss"] = cfg.pred_normal_loss_mult * torch.mean(outputs["rendered_pred_normal_loss"])
        return out

    def get_loss_dict(self, outputs, batch, metrics_dict=None) -> dict:
        """nerfstudio's NerfactoModel.get_loss_dict [NS-RECALL]: ``rgb_loss`` (MSE) and, while training, ``interlevel_loss`` and
        ``distortion_loss`` from ``outputs["weights_list"]`` / ``outputs["ray_samples_list"]`` (last entry: the main level)."""
        loss_dict = {"rgb_loss": torch.mean((self._gt_rgb(batch) - outputs["rgb"]) ** 2)}
        if self.training:
            loss_dict.update(self._sampler_losses(outputs, metrics_dict))
        return loss_dict

    # nerfstudio's MLPWithHashEncoding may register its torch-path pair as `model = nn.Sequential(encoder, mlp)` [NS-RECALL, M] -- a checkpoint then
    # holds `<...>.mlp_base.model.0.hash_table` / `<...>.mlp_base.model.1.layers.N.{weight,bias}` instead of (or beside) the `encoder.` / `mlp.` names
    # this package uses.  Both spellings load: an alias is renamed when its canonical key is absent and dropped when it is present (same tensor).
    _KEY_ALIASES = ((re.compile(r"^(.*\.mlp_base)\.model\.0\.(hash_table)$"), r"\1.encoder.\2"),
                    (re.compile(r"^(.*\.mlp_base)\.model\.1\.(layers\.\d+\.(?:weight|bias))$"), r"\1.mlp.\2"))

    @classmethod
    def _canonical_keys(cls, state_dict):
        out = {}
        for k, v in state_dict.items():
            for pat, rep in cls._KEY_ALIASES:
                if pat.match(k):
                    canon = pat.sub(rep, k)
                    if canon not in state_dict:
                        out[canon] = v
                    break
            else:
                out[k] = v
        return out

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        if any(k.endswith(".params") for k in state_dict):  # a tiny-cuda-nn checkpoint (flat parameter vectors)
            from .tcnn_import import convert_tcnn_state_dict

            state_dict = convert_tcnn_state_dict(state_dict, self.config)
        state_dict = self._canonical_keys(state_dict)
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._weights_dirty = True
        # strict=False is how the reference loads (signerf_pipeline.py:131): a FIELD parameter that is not in the checkpoint keeps its random
        # initialisation without a word from torch, and the render is noise.  The keys the reference strips on purpose are not reported: the
        # appearance table, the camera optimiser -- and the proposal nets when ALL of them are gone, which is SIGNeRFPipeline's default load
        # (load_model_with_proposal_weights=False deletes every `proposal*` key, :126-129; ADVICE r04: that normal flow must not warn).  A
        # checkpoint that holds SOME proposal keys and misses others is reported like a missing field parameter.
        prop_keys = [k for k in self.state_dict() if k.startswith("proposal_networks.")]
        prop_missing = [k for k in out.missing_keys if k.startswith("proposal_networks.")]
        stripped = len(prop_missing) == len(prop_keys)
        lost = [k for k in out.missing_keys if k.startswith(("field.mlp_base.", "field.mlp_head.")) or (not stripped and k.startswith("proposal_networks."))]
        if lost:
            mods = sorted({".".join(k.split(".")[:3 if k.startswith("proposal") else 2]) for k in lost})
            warnings.warn(f"load_state_dict: {len(lost)} render parameters are not in the state dict and keep their random initialisation "
                          f"({', '.join(mods)}; e.g. {lost[0]!r}) -- renders through these modules are meaningless until they are loaded",
                          RuntimeWarning, stacklevel=2)
        return out

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self._weights_dirty = True
        return out

    def mark_weights_dirty(self):
        """Call after mutating parameters in place (e.g. an optimizer step) so the next render re-uploads them."""
        self._weights_dirty = True

    # -- HIP engine (signerf_amd.engine): what code outside the package calls on the model ------------------------
    @property
    def _weights_dirty(self) -> bool:
        return self._engine.dirty

    @_weights_dirty.setter
    def _weights_dirty(self, value: bool) -> None:
        self._engine.dirty = value

    @property
    def effective_precision(self) -> str:
        """What ``config.precision`` resolves to for the uploaded parameters (``Engine.effective_precision``)."""
        return self._engine.effective_precision()

    def _ensure_engine(self):
        return self._engine.ensure()

    def _render_normals(self, b: RayBundle, H: int, W: int, state=None) -> Dict[str, Tensor]:
        return self._engine.render_normals(b, H, W, state)

    # for tests that call the C entry points themselves, single-threaded, on a model that has rendered (they predate the engine)
    @property
    def _handle(self):
        return self._engine.handle

    def _opts(self, H: int, W: int, lib, single_chunk: bool = False):
        return self._engine.opts(lib, self._engine.handle, H, W, single_chunk)

    def __del__(self):
        try:
            self._engine.close()
        except Exception:
            pass

    def _field_desc(self) -> _lib.SnFieldDesc:
        cfg = self.config
        d = _lib.SnFieldDesc()
        d.main_field = _desc_of(self.field.mlp_base.encoder, cfg.hidden_dim, 1 + self.field.geo_feat_dim)
        d.geo_feat_dim = self.field.geo_feat_dim
        d.hidden_dim_color = cfg.hidden_dim_color
        d.appearance_embed_dim = cfg.appearance_embed_dim
        d.sh_levels = 4
        d.sh_remap = 0 if cfg.implementation == "torch" else 1
        d.num_proposals = len(self.proposal_networks)
        for i, net in enumerate(self.proposal_networks):
            d.proposals[i] = _desc_of(net.mlp_base.encoder, net.mlp_base.mlp.layers[0].out_features, 1)
        d.average_init_density = cfg.average_init_density
        d.histogram_padding = 0.01
        # nerfacto.py (nerfstudio): disable_scene_contraction -> the fields normalise positions with the model's scene box instead
        # (SceneBox.get_normalized_positions); nerfstudio's dataparsers hand out [-1, 1]^3 x scene_scale, the default here
        d.disable_scene_contraction = 1 if cfg.disable_scene_contraction else 0
        aabb = self.scene_box.aabb if self.scene_box is not None else torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
        for k, v in enumerate(aabb.detach().to(torch.float32).cpu().reshape(6).tolist()):
            d.aabb[k] = v
        d.dense_levels = int(getattr(cfg, "dense_levels", 0))
        d.dense_copy_cap_mb = int(getattr(cfg, "dense_copy_cap_mb", 0))
        d.half_grid = 1 if wants_half_grid(cfg) else 0
        return d

    # -- rows a6-a17 ---------------------------------------------------------------------------------------------
    @torch.no_grad()
    def get_outputs_for_camera_ray_bundle(self, camera_ray_bundle: RayBundle) -> Dict[str, Tensor]:
        """Whole-image render: dict of [H,W,C] fp32 tensors on the bundle's device ("rgb", "accumulation", "depth"
        (median), "expected_depth", "prop_depth_i").  Rays are visited in the reference's row-major order; the
        reference's 32 768-ray chunking only survives in the expected-depth clip bounds (A17)."""
        H, W = camera_ray_bundle.origins.shape[:2]
        return self._with_normals(camera_ray_bundle, H, W, (H, W))

    @torch.no_grad()
    def get_outputs_for_camera(self, camera, obb_box=None) -> Dict[str, Tensor]:
        """nerfstudio's ``Model.get_outputs_for_camera`` [NS], the call the viewer's render thread makes on the shared model
        (/root/reference/signerf/interface/viewer.py:334-336): rays of camera 0, then the whole-image
        render -- the same kernels at the viewer's resolution.  ``obb_box`` (the viewer's crop box) bounds the rays through
        nerfstudio's ``intersect_obb`` (``Cameras.generate_rays(obb_box=...)``)."""
        return self.get_outputs_for_camera_ray_bundle(camera.generate_rays(camera_indices=0, aabb_box=self.render_aabb, obb_box=obb_box))

    @torch.no_grad()
    def get_outputs(self, ray_bundle: RayBundle) -> Dict[str, Tensor]:
        """Flat bundle [R,...] -> dict of [R,C]."""
        R = len(ray_bundle)
        return self._with_normals(ray_bundle.flatten(), 1, R, (R,), single_chunk=True)

    def forward(self, ray_bundle: RayBundle) -> Dict[str, Tensor]:
        if self.training and self.config.training_forward:
            return self.get_training_outputs(ray_bundle)
        return self.get_outputs(ray_bundle)

    # -- training forward -----------------------------------------------------------------------------------------
    def _training_sampler(self):
        """The training-mode ``ProposalNetworkSampler`` of this model's config (signerf_amd.samplers), made on first use.  Its Philox seed
        is 0; set ``model._training_sampler().seed`` before the first step for another stream."""
        sampler = self.__dict__.get("_train_sampler")
        if sampler is None:
            from . import samplers

            cfg = self.config
            n = cfg.num_proposal_iterations
            if n < 1:
                raise NotImplementedError("training forward: num_proposal_iterations >= 1 expected")
            sampler = samplers.ProposalNetworkSampler(
                num_nerf_samples_per_ray=cfg.num_nerf_samples_per_ray, num_proposal_samples_per_ray=tuple(cfg.num_proposal_samples_per_ray[:n]),
                num_proposal_network_iterations=n, single_jitter=cfg.use_single_jitter,
                update_sched=samplers.update_schedule(cfg.proposal_warmup, cfg.proposal_update_every),
                initial_sampler=cfg.proposal_initial_sampler, seed=0, near_plane=cfg.near_plane, far_plane=cfg.far_plane)
            self.__dict__["_train_sampler"] = sampler
        return sampler

    def set_training_step(self, step: int) -> None:
        """What nerfstudio's two training callbacks do before a step: the proposal-weight anneal
        ``bias(clip(step / N, 0, 1), slope)``, ``bias(x, b) = b x / ((b - 1) x + 1)``, and the sampler's ``step_cb``.
        (``get_training_callbacks`` stays empty: a trainer of this package calls this itself.)"""
        from . import samplers

        cfg = self.config
        sampler = self._training_sampler()
        if cfg.use_proposal_weight_anneal:
            sampler.set_anneal(samplers.anneal_at(step, cfg.proposal_weights_anneal_slope, cfg.proposal_weights_anneal_max_num_iters))
        sampler.step_cb(step)

    def get_training_outputs(self, ray_bundle: RayBundle) -> Dict:
        """nerfstudio's training ``NerfactoModel.get_outputs`` [NS-RECALL]: training-mode proposal sampling (HIP, signerf_amd.samplers), the
        proposal networks and the field as differentiable torch ops around the HIP hash grid (``get_density_training`` /
        ``forward_training``), differentiable compositing (HIP, ``losses.composite``).  Flat bundle [R, ...] ->
        ``rgb`` [R,3], ``accumulation`` [R,1], ``depth`` (median) / ``expected_depth`` [R,1] (no gradient), ``weights_list`` and
        ``ray_samples_list`` (last entry: the main level) and ``prop_depth_i`` [R,1]; with ``config.training_normals`` on a
        ``predict_normals`` model also ``normals`` / ``pred_normals`` [R,3] (shaded, no gradient), ``rendered_orientation_loss`` [R] (no
        gradient) and ``rendered_pred_normal_loss`` [R] (HIP, ``signerf_amd.train_normals``).  Whatever the model's mode.  The parameters are
        read where they live, not through the HIP handle: ``mark_weights_dirty()`` after an optimizer step, before the next eval render."""
        from . import losses

        cfg = self.config
        bg = BACKGROUNDS[cfg.background_color]
        if cfg.background_color == "random":
            raise NotImplementedError('training forward: background_color="random" (a fresh colour per ray) is not built; "last_sample", '
                                      '"black" or "white" expected')
        b = ray_bundle.flatten()
        ray_samples, weights_list, ray_samples_list = self._training_sampler()(b, [net.get_density_training for net in self.proposal_networks])
        with_normals = cfg.training_normals and cfg.predict_normals
        field = self.field.forward_training(ray_samples, appearance="per_camera" if b.camera_indices is not None else "mean",
                                            compute_normals=with_normals)
        background = "last_sample" if bg is None else torch.tensor(bg, dtype=torch.float32, device=b.origins.device)
        weights, rgb, accumulation = losses.composite(field[FieldHeadNames.DENSITY], field[FieldHeadNames.RGB], ray_samples.deltas, background)
        weights_list.append(weights)
        ray_samples_list.append(ray_samples)
        outputs = {"rgb": rgb, "accumulation": accumulation}
        if with_normals:
            from . import train_normals

            # nerfacto hands both losses the weights and the analytic normals detached; the shaded normals carry no gradient here (in
            # nerfstudio they are differentiable in the weights, but no loss reads them)
            orientation, pred_normal, normals, pred_normals = train_normals._normal_terms(
                weights.detach(), field[FieldHeadNames.NORMALS], field[FieldHeadNames.PRED_NORMALS], b.directions)
            outputs.update({"normals": normals, "pred_normals": pred_normals, "rendered_orientation_loss": orientation,
                            "rendered_pred_normal_loss": pred_normal})
        with torch.no_grad():
            outputs["depth"] = _median_depth(weights, ray_samples)
            outputs["expected_depth"] = _expected_depth(weights, ray_samples)
            for i in range(cfg.num_proposal_iterations):
                outputs[f"prop_depth_{i}"] = _median_depth(weights_list[i], ray_samples_list[i])
        outputs["weights_list"] = weights_list
        outputs["ray_samples_list"] = ray_samples_list
        return outputs

    def _with_normals(self, b: RayBundle, H: int, W: int, shape, single_chunk: bool = False) -> Dict[str, Tensor]:
        mode = self.config.compute_normals if self.config.predict_normals else "never"
        if mode not in ("lazy", "always", "never"):
            raise ValueError(f"compute_normals must be 'lazy', 'always' or 'never', got {mode!r}")
        # Behind the proposal sampler the normals kernel marches the SAME final bins as the colour render: the render's workspace (which
        # holds them) stays alive with the outputs, and the normals launch reads it instead of running the proposal kernel a second time
        # (SnRenderOpts.reuse_final_bins; 17.5 -> 10 ms at 1920x1080).  The price: that workspace is released when the outputs dict
        # is, not when this call returns.
        keep_bins = mode != "never" and self.config.num_proposal_iterations > 0 and H * W > 0
        # lazy mode: only below config.normals_bin_reuse_max_mb (the workspace then lives as long as the outputs dict does)
        cap = None if mode == "always" else int(self.config.normals_bin_reuse_max_mb) << 20
        raw, state = self._engine.render(b, H, W, single_chunk, keep_state=keep_bins, keep_state_max_bytes=cap)
        out = {k: v.view(*shape, v.shape[-1]) for k, v in raw.items()}
        if mode == "never":
            return out

        held = [state]   # released with the first (only) normals launch, not with the outputs dict

        def producer():
            with torch.no_grad():
                st, held[0] = held[0], None
                return {k: v.view(*shape, v.shape[-1]) for k, v in self._render_normals(b, H, W, st).items()}

        if mode == "always":
            out.update(producer())
            return out
        return LazyOutputs(out, producer)


class SIGNeRFModel(NerfactoModel):
    """signerf.py:27-82: the same render path; the training losses differ."""

    config: SIGNeRFModelConfig

    def populate_modules(self):
        super().populate_modules()
        # The perceptual metric of the LPIPS term, ``lpips(pred, target)`` on [N, 3, patch, patch] images in [-1, 1] -> a scalar.  Its
        # weights are not shipped: attach a module (``model.lpips = LearnedPerceptualImagePatchSimilarity()`` of torchmetrics, as
        # signerf.py:39 does) or set ``use_lpips=False``.
        self.lpips = None

    def get_loss_dict(self, outputs, batch, metrics_dict=None) -> dict:
        """signerf.py:41-82: L1 (``use_l1``) or MSE on the rgb, the LPIPS term on ``patch_size`` x ``patch_size`` patches normalised to
        [-1, 1], and while training the sampler losses."""
        cfg = self.config
        image, output = self._gt_rgb(batch), outputs["rgb"]
        loss_dict = {"rgb_loss": torch.mean(torch.abs(image - output)) if cfg.use_l1 else torch.mean((image - output) ** 2)}
        if cfg.use_lpips:
            lpips = getattr(self, "lpips", None)
            if lpips is None:
                raise NotImplementedError("use_lpips=True, but LPIPS weights are not shipped with this package: attach a module that maps "
                                          "(pred, target) patches [N, 3, patch, patch] in [-1, 1] to a scalar as `model.lpips = ...` "
                                          "(torchmetrics' LearnedPerceptualImagePatchSimilarity), or set use_lpips=False")
            ps = cfg.patch_size
            out_patches = (output.reshape(-1, ps, ps, 3).permute(0, 3, 1, 2) * 2 - 1).clamp(-1, 1)
            gt_patches = (image.reshape(-1, ps, ps, 3).permute(0, 3, 1, 2) * 2 - 1).clamp(-1, 1)
            loss_dict["lpips_loss"] = cfg.lpips_loss_mult * lpips(out_patches, gt_patches)
        if self.training:
            loss_dict.update(self._sampler_losses(outputs, metrics_dict))
        return loss_dict
