"""The back half of a training step: differentiable compositing and nerfacto's two sampler losses, in HIP (include/signerf_hip_losses.h,
csrc/sn_losses.h), behind ``torch.autograd.Function`` wrappers with nerfstudio's names and shapes [NS-RECALL, nerfstudio 1.0.2:
``RaySamples.get_weights``, ``RGBRenderer`` / ``AccumulationRenderer`` in training mode, ``model_components/losses.py``].

Everything here runs AFTER the field has produced per-sample densities and colours; of the field itself the hash encoding is a HIP op
(``signerf_amd.hashgrid``) and the rest torch ops; the training-mode sampling that produces ``weights_list`` / ``ray_samples_list`` is
``signerf_amd.samplers`` (DESIGN.md §4 "Training back half", "Training-mode sampling").

Inputs are fp32 GPU tensors: another dtype raises ``TypeError``, a CPU tensor raises ``SignerfHipError`` (there is no CPU path), a
non-contiguous tensor is made contiguous.  What gets a gradient:

* ``get_weights`` / ``composite``: the densities and the colours.  NOT the deltas -- nerfacto's samplers hand out detached bins -- and not
  a constant background colour.
* ``lossfun_distortion``: ``w``; ``t`` is a constant.
* ``lossfun_outer``: ``w_env`` only; ``t``, ``w`` and ``t_env`` are detached in nerfacto's interlevel loss.

Means over rays are taken by torch on the kernels' per-ray vectors.
"""

from __future__ import annotations

from typing import List, Optional, Tuple, Union

import torch
from torch import Tensor

from . import _lib


TAKES = "the loss kernels are fp32 in, fp64 inside, fp32 out"


def _grad(g: Optional[Tensor]) -> Optional[Tensor]:
    return None if g is None else g.to(torch.float32).contiguous()


class _Composite(torch.autograd.Function):
    """(density [R,S], colour [R,S,3] | None, deltas [R,S], background [3] | None) -> weights [R,S], rgb [R,3], accumulation [R,1]."""

    @staticmethod
    def forward(ctx, density, colour, deltas, background):
        R, S = density.shape
        dev = density.device
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(density, colour, deltas, background)
        with torch.cuda.device(dev):
            weights = torch.empty((R, S), dtype=torch.float32, device=dev)
            rgb = torch.empty((R, 3), dtype=torch.float32, device=dev) if colour is not None else None
            acc = torch.empty((R, 1), dtype=torch.float32, device=dev)
            if R > 0:
                lib = _lib.load()
                _lib.check(lib.sn_loss_composite_forward(_lib.ptr(deltas), _lib.ptr(density), _lib.ptr(colour), _lib.ptr(background), R, S,
                                                         _lib.ptr(weights), _lib.ptr(rgb), _lib.ptr(acc), _lib.current_stream()),
                           None, "sn_loss_composite_forward")
        if rgb is None:
            rgb = torch.empty((R, 0), dtype=torch.float32, device=dev)
            ctx.mark_non_differentiable(rgb)
        return weights, rgb, acc

    @staticmethod
    def backward(ctx, g_weights, g_rgb, g_acc):
        density, colour, deltas, background = ctx.saved_tensors
        R, S = density.shape
        dev = density.device
        if colour is None:
            g_rgb = None
        g_weights, g_rgb, g_acc = _grad(g_weights), _grad(g_rgb), _grad(g_acc)
        with torch.cuda.device(dev):
            g_density = torch.empty((R, S), dtype=torch.float32, device=dev)
            g_colour = torch.empty((R, S, 3), dtype=torch.float32, device=dev) if (colour is not None and ctx.needs_input_grad[1]) else None
            if R > 0:
                lib = _lib.load()
                _lib.check(lib.sn_loss_composite_backward(_lib.ptr(deltas), _lib.ptr(density), _lib.ptr(colour), _lib.ptr(background), R, S,
                                                          _lib.ptr(g_weights), _lib.ptr(g_rgb), _lib.ptr(g_acc), _lib.ptr(g_density),
                                                          _lib.ptr(g_colour), _lib.current_stream()),
                           None, "sn_loss_composite_backward")
        return g_density, g_colour, None, None


class _Distortion(torch.autograd.Function):
    """(t [R,S+1], w [R,S]) -> loss [R]."""

    @staticmethod
    def forward(ctx, t, w):
        R, S = w.shape
        ctx.save_for_backward(t, w)
        with torch.cuda.device(w.device):
            loss = torch.empty((R,), dtype=torch.float32, device=w.device)
            if R > 0:
                _lib.check(_lib.load().sn_loss_distortion_forward(_lib.ptr(t), _lib.ptr(w), R, S, _lib.ptr(loss), _lib.current_stream()),
                           None, "sn_loss_distortion_forward")
        return loss

    @staticmethod
    def backward(ctx, g):
        t, w = ctx.saved_tensors
        R, S = w.shape
        g = _grad(g)
        with torch.cuda.device(w.device):
            g_w = torch.empty((R, S), dtype=torch.float32, device=w.device)
            if R > 0:
                _lib.check(_lib.load().sn_loss_distortion_backward(_lib.ptr(t), _lib.ptr(w), _lib.ptr(g), R, S, _lib.ptr(g_w),
                                                                   _lib.current_stream()), None, "sn_loss_distortion_backward")
        return None, g_w


class _Interlevel(torch.autograd.Function):
    """(t [R,S+1], w [R,S], t_env [R,P+1], w_env [R,P]) -> per-ray mean loss [R]."""

    @staticmethod
    def forward(ctx, t, w, t_env, w_env):
        R, S = w.shape
        P = w_env.shape[1]
        ctx.save_for_backward(t, w, t_env, w_env)
        with torch.cuda.device(w.device):
            loss = torch.empty((R,), dtype=torch.float32, device=w.device)
            if R > 0:
                _lib.check(_lib.load().sn_loss_interlevel_forward(_lib.ptr(t), _lib.ptr(w), _lib.ptr(t_env), _lib.ptr(w_env), R, S, P,
                                                                  _lib.ptr(loss), None, _lib.current_stream()), None,
                           "sn_loss_interlevel_forward")
        return loss

    @staticmethod
    def backward(ctx, g):
        t, w, t_env, w_env = ctx.saved_tensors
        R, S = w.shape
        P = w_env.shape[1]
        g = _grad(g)
        with torch.cuda.device(w.device):
            g_env = torch.empty((R, P), dtype=torch.float32, device=w.device)
            if R > 0:
                _lib.check(_lib.load().sn_loss_interlevel_backward(_lib.ptr(t), _lib.ptr(w), _lib.ptr(t_env), _lib.ptr(w_env), _lib.ptr(g), R, S,
                                                                   P, _lib.ptr(g_env), _lib.current_stream()), None, "sn_loss_interlevel_backward")
        return None, None, None, g_env


def _check_samples(S: int, what: str) -> None:
    if not 1 <= S <= 1024:
        raise ValueError(f"{what}: 1..1024 samples per ray expected, got {S}")


def _rows(x: Tensor, last: int) -> Tensor:
    """[..., S, last] -> [R, S] (last == 1) or [R, S, last]."""
    S = x.shape[-2]
    return x.reshape(-1, S) if last == 1 else x.reshape(-1, S, last)


def get_weights(deltas: Tensor, densities: Tensor) -> Tensor:
    """``RaySamples.get_weights``: deltas, densities [..., S, 1] -> weights [..., S, 1] = nan_to_num(alpha_i T_i)."""
    deltas, densities = _lib.prep(deltas, "deltas", TAKES), _lib.prep(densities, "densities", TAKES)
    if deltas.shape != densities.shape or deltas.ndim < 2 or deltas.shape[-1] != 1:
        raise ValueError(f"get_weights: deltas and densities [..., S, 1] expected, got {tuple(deltas.shape)} and {tuple(densities.shape)}")
    _check_samples(deltas.shape[-2], "get_weights")
    weights, _, _ = _Composite.apply(_rows(densities, 1), None, _rows(deltas, 1).detach(), None)
    return weights.reshape(densities.shape)


def composite(densities: Tensor, rgbs: Tensor, deltas: Tensor,
              background_color: Union[str, Tensor] = "last_sample") -> Tuple[Tensor, Tensor, Tensor]:
    """The fused form of ``get_weights`` + ``RGBRenderer`` + ``AccumulationRenderer``, training semantics (no clamp and no nan_to_num on the
    colours): densities, deltas [..., S, 1], rgbs [..., S, 3] -> (weights [..., S, 1], rgb [..., 3], accumulation [..., 1]).
    ``background_color``: "last_sample" (nerfacto's default; its dependence on the last sample's colour is differentiated) or a constant
    colour, a Tensor [3]."""
    densities, rgbs, deltas = _lib.prep(densities, "densities", TAKES), _lib.prep(rgbs, "rgbs", TAKES), _lib.prep(deltas, "deltas", TAKES)
    if deltas.shape != densities.shape or deltas.ndim < 2 or deltas.shape[-1] != 1 or rgbs.shape != (*densities.shape[:-1], 3):
        raise ValueError(f"composite: densities, deltas [..., S, 1] and rgbs [..., S, 3] expected, got {tuple(densities.shape)}, "
                         f"{tuple(deltas.shape)}, {tuple(rgbs.shape)}")
    _check_samples(deltas.shape[-2], "composite")
    if isinstance(background_color, str):
        if background_color != "last_sample":
            raise ValueError(f'background_color={background_color!r}: "last_sample" or a Tensor [3] expected')
        bg = None
    else:
        bg = _lib.prep(background_color, "background_color", TAKES).detach()
        if bg.shape != (3,):
            raise ValueError(f"background_color: a Tensor [3] expected, got {tuple(bg.shape)}")
    lead = densities.shape[:-2]
    weights, rgb, acc = _Composite.apply(_rows(densities, 1), _rows(rgbs, 3), _rows(deltas, 1).detach(), bg)
    return weights.reshape(densities.shape), rgb.reshape(*lead, 3), acc.reshape(*lead, 1)


def ray_samples_to_sdist(ray_samples) -> Tensor:
    """The S + 1 normalised bin edges of S samples: ``spacing_starts`` with the last of ``spacing_ends`` appended, [..., S+1]."""
    if ray_samples.spacing_starts is None or ray_samples.spacing_ends is None:
        raise ValueError("ray_samples_to_sdist: the ray samples carry no spacing_starts / spacing_ends")
    return torch.cat([ray_samples.spacing_starts[..., 0], ray_samples.spacing_ends[..., -1:, 0]], dim=-1)


def lossfun_distortion(t: Tensor, w: Tensor) -> Tensor:
    """mip-NeRF 360's distortion loss of a step function: t [..., S+1] edges, w [..., S] weights -> [...], one value per ray."""
    t, w = _lib.prep(t, "t", TAKES), _lib.prep(w, "w", TAKES)
    if t.ndim < 1 or w.ndim < 1 or t.shape[:-1] != w.shape[:-1] or t.shape[-1] != w.shape[-1] + 1:
        raise ValueError(f"lossfun_distortion: t [..., S+1] and w [..., S] expected, got {tuple(t.shape)} and {tuple(w.shape)}")
    S = w.shape[-1]
    _check_samples(S, "lossfun_distortion")
    return _Distortion.apply(t.reshape(-1, S + 1).detach(), w.reshape(-1, S)).reshape(w.shape[:-1])


def lossfun_outer(t: Tensor, w: Tensor, t_env: Tensor, w_env: Tensor) -> Tensor:
    """The proposal loss of one level: how far the histogram (t, w) [..., S+1], [..., S] pokes out of its envelope (t_env, w_env)
    [..., P+1], [..., P].  Returns the per-ray MEAN over the S samples, [...] (nerfstudio's function returns the [..., S] terms and its
    caller takes the mean over everything; with equal S per ray the two agree).  Only ``w_env`` gets a gradient."""
    t, w, t_env, w_env = _lib.prep(t, "t", TAKES), _lib.prep(w, "w", TAKES), _lib.prep(t_env, "t_env", TAKES), _lib.prep(w_env, "w_env", TAKES)
    lead = w.shape[:-1]
    if (t.shape[:-1] != lead or t_env.shape[:-1] != lead or w_env.shape[:-1] != lead or t.shape[-1] != w.shape[-1] + 1
            or t_env.shape[-1] != w_env.shape[-1] + 1):
        raise ValueError(f"lossfun_outer: t [..., S+1], w [..., S], t_env [..., P+1], w_env [..., P] expected, got {tuple(t.shape)}, "
                         f"{tuple(w.shape)}, {tuple(t_env.shape)}, {tuple(w_env.shape)}")
    S, P = w.shape[-1], w_env.shape[-1]
    _check_samples(S, "lossfun_outer (S)")
    _check_samples(P, "lossfun_outer (P)")
    return _Interlevel.apply(t.reshape(-1, S + 1).detach(), w.reshape(-1, S).detach(), t_env.reshape(-1, P + 1).detach(),
                             w_env.reshape(-1, P)).reshape(lead)


def outer(t: Tensor, t_env: Tensor, w_env: Tensor) -> Tensor:
    """nerfstudio's ``outer``: for every interval of t [..., S+1] the sum of the envelope's weights w_env [..., P] over the intervals of
    t_env [..., P+1] it touches, [..., S].  For inspection and tests: no gradient."""
    t, t_env, w_env = _lib.prep(t, "t", TAKES).detach(), _lib.prep(t_env, "t_env", TAKES).detach(), _lib.prep(w_env, "w_env", TAKES).detach()
    lead = w_env.shape[:-1]
    if t.shape[:-1] != lead or t_env.shape[:-1] != lead or t_env.shape[-1] != w_env.shape[-1] + 1 or t.shape[-1] < 2:
        raise ValueError(f"outer: t [..., S+1], t_env [..., P+1], w_env [..., P] expected, got {tuple(t.shape)}, {tuple(t_env.shape)}, "
                         f"{tuple(w_env.shape)}")
    S, P = t.shape[-1] - 1, w_env.shape[-1]
    _check_samples(S, "outer (S)")
    _check_samples(P, "outer (P)")
    R = w_env.numel() // P
    with torch.cuda.device(t.device):
        out = torch.empty((*lead, S), dtype=torch.float32, device=t.device)
        if R > 0:
            _lib.check(_lib.load().sn_loss_interlevel_forward(_lib.ptr(t), None, _lib.ptr(t_env), _lib.ptr(w_env), R, S, P, None, _lib.ptr(out),
                                                              _lib.current_stream()), None, "sn_loss_interlevel_forward")
    return out


def distortion_loss(weights_list: List[Tensor], ray_samples_list: List) -> Tensor:
    """nerfstudio's ``distortion_loss``: the mean over rays of ``lossfun_distortion`` of the main (last) level."""
    c = ray_samples_to_sdist(ray_samples_list[-1])
    w = weights_list[-1][..., 0]
    return torch.mean(lossfun_distortion(c, w))


def interlevel_loss(weights_list: List[Tensor], ray_samples_list: List) -> Tensor:
    """nerfstudio's ``interlevel_loss``: the last list entry is the main level (detached); the sum over the proposal levels of the mean
    over rays of the per-ray means of ``lossfun_outer``."""
    c = ray_samples_to_sdist(ray_samples_list[-1]).detach()
    w = weights_list[-1][..., 0].detach()
    assert len(ray_samples_list) > 0
    loss = 0.0
    for ray_samples, weights in zip(ray_samples_list[:-1], weights_list[:-1]):
        loss = loss + torch.mean(lossfun_outer(c, w, ray_samples_to_sdist(ray_samples), weights[..., 0]))
    return loss
