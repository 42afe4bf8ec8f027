"""The normals half of a training step, in HIP: the analytic normals of training samples (include/signerf_hip_train_normals.h,
csrc/sn_train_normals.h) and the per-ray normal terms -- nerfstudio's ``orientation_loss`` and ``pred_normal_loss`` and the rendered
normals (include/signerf_hip_normal_losses.h, csrc/sn_normal_losses.h) [NS-RECALL, nerfstudio 1.0.2: ``Field.get_normals``,
``model_components/losses.py``, ``NormalsRenderer`` / ``NormalsShader``].  DESIGN.md §4 "Training-mode normals".

nerfstudio's analytic normals are constants for autograd: ``Field.get_normals`` calls ``torch.autograd.grad`` on the pre-activation
density without ``create_graph``, and nerfacto hands the weights and those normals to both losses detached.  So ``analytic_normals`` builds
no graph, the orientation term is a reported value, and the only gradient anywhere here is the pred-normal term's in the predicted normals.

Inputs are fp32 GPU tensors: another dtype raises ``TypeError``, a CPU tensor raises ``SignerfHipError`` (there is no CPU path), a
non-contiguous tensor is made contiguous; a shape that does not fit raises ``ValueError``.  No atomics anywhere: every result is
bit-reproducible from call to call.
"""

from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib, hashgrid, mlp


def _check_points(q, hash_table, scalings, log2_hashmap_size, weights, biases, who: str):
    """hashgrid's and mlp's own checks in their order (every dtype, then every device, then shapes), and dims[0] == L * F."""
    weights, biases = list(weights), list(biases)
    for x, name in ((q, "q"), (hash_table, "hash_table"), (scalings, "scalings")):
        _lib.typed(x, name, hashgrid.TAKES)
    for i, w in enumerate(weights):
        _lib.typed(w, f"weights[{i}]", mlp.TAKES)
    for i, b in enumerate(biases):
        _lib.typed(b, f"biases[{i}]", mlp.TAKES)
    for x, name in ((q, "q"), (hash_table, "hash_table"), (scalings, "scalings")):   # every device before any shape
        if not x.is_cuda:
            raise _lib.SignerfHipError(f"{name} must live on the GPU (there is no CPU path)")
    weights = [_lib.prep(w, f"weights[{i}]", mlp.TAKES).detach() for i, w in enumerate(weights)]
    biases = [_lib.prep(b, f"biases[{i}]", mlp.TAKES).detach() for i, b in enumerate(biases)]
    q, hash_table, scalings = hashgrid._check(q, hash_table, scalings, log2_hashmap_size)
    if len(weights) != len(biases) or not weights:
        raise ValueError(f"{who}: as many weights as biases, at least one, expected; got {len(weights)} and {len(biases)}")
    dims = [scalings.numel() * hash_table.shape[1]]
    for i, (w, b) in enumerate(zip(weights, biases)):
        if w.ndim != 2 or w.shape[1] != dims[-1] or b.shape != (w.shape[0],):
            raise ValueError(f"{who}: weights[{i}] [out, {dims[-1]}] and biases[{i}] [out] expected (weights[0] takes the L * F features of "
                             f"the encoding), got {tuple(w.shape)} and {tuple(b.shape)}")
        if w.device != q.device or b.device != q.device:
            raise ValueError(f"{who}: q and every parameter on one device expected, got {q.device}, {w.device}, {b.device}")
        dims.append(w.shape[0])
    mlp.check_dims(dims)
    if q.numel() // 3 >= 2**31:
        raise ValueError(f"{who}: fewer than 2**31 points expected")
    return q.detach(), hash_table.detach(), scalings, weights, biases, dims


def analytic_normals(q: Tensor, hash_table: Tensor, scalings: Tensor, log2_hashmap_size: int, weights: Sequence[Tensor],
                     biases: Sequence[Tensor], return_grad: bool = False):
    """nerfstudio's ``Field.get_normals`` for the field ``mlp(hash_encode(q))``: ``-g / max(|g|, 1e-12)`` with ``g`` the gradient of the
    stack's output channel 0 (the pre-activation density) in ``q``.  q [..., 3], the hash grid as ``hashgrid.hash_encode`` takes it, the
    stack as ``mlp.fused_mlp`` takes it with ``weights[0]`` [*, L * F] -> normals [..., 3], or (normals, g) with ``return_grad``.  One HIP
    kernel; no autograd graph, the result does not require a gradient.  A zero gradient gives a zero normal; an out-of-domain point
    (``signerf_amd.hashgrid``) a NaN one."""
    q, hash_table, scalings, weights, biases, dims = _check_points(q, hash_table, scalings, log2_hashmap_size, weights, biases, "analytic_normals")
    N, L, F = q.numel() // 3, scalings.numel(), hash_table.shape[1]
    with torch.cuda.device(q.device):
        normals = torch.empty_like(q)
        grad = torch.empty_like(q) if return_grad else None
        if N > 0:
            _lib.check(_lib.load().sn_train_normals_analytic(_lib.ptr(q), _lib.ptr(hash_table), _lib.ptr(scalings), N, L, log2_hashmap_size, F,
                                                             C.byref(mlp._desc(dims, weights, biases)), _lib.ptr(normals), _lib.ptr(grad),
                                                             _lib.current_stream()), None, "sn_train_normals_analytic")
    return (normals, grad) if return_grad else normals


def analytic_normals_composed(q: Tensor, hash_table: Tensor, scalings: Tensor, log2_hashmap_size: int, weights: Sequence[Tensor],
                              biases: Sequence[Tensor], return_grad: bool = False):
    """The same quantity by the two existing launches -- ``mlp.mlp_backward`` of the one-hot gradient on the encoding, then
    ``hashgrid.hash_encode_backward(want_grad_q=True)`` -- and torch's ``F.normalize``.  Same arguments, same result up to rounding.  The
    tests' second witness and the other side of tools/train_normals_bench.py; the field calls ``analytic_normals``, which is 2.3 times
    faster on its shape (DESIGN.md §4 "Training-mode normals", "Measurement")."""
    q, hash_table, scalings, weights, biases, dims = _check_points(q, hash_table, scalings, log2_hashmap_size, weights, biases,
                                                                   "analytic_normals_composed")
    flat = q.reshape(-1, 3)
    enc = hashgrid.hash_encode(flat, hash_table, scalings, log2_hashmap_size)
    one_hot = torch.zeros((flat.shape[0], dims[-1]), dtype=torch.float32, device=q.device)
    one_hot[:, 0] = 1.0
    g_enc, _, _ = mlp.mlp_backward(enc, weights, biases, one_hot, want_grad_x=True, want_grad_params=False)
    _, g = hashgrid.hash_encode_backward(flat, hash_table, scalings, log2_hashmap_size, g_enc, want_grad_q=True)
    normals = (-torch.nn.functional.normalize(g, dim=-1)).reshape(q.shape)
    return (normals, g.reshape(q.shape)) if return_grad else normals


# ---- the per-ray terms ----------------------------------------------------------------------------------------------------------------------
def _forward(weights, normals, pred_normals, directions, want: Tuple[bool, bool, bool, bool]):
    """[R,S], [R,S,3], [R,S,3] | None, [R,3] | None -> the four outputs of sn_loss_normals_forward, None where not wanted."""
    R, S = weights.shape
    dev = weights.device
    with torch.cuda.device(dev):
        outs = [torch.empty(shape, dtype=torch.float32, device=dev) if w else None for w, shape in zip(want, ((R,), (R,), (R, 3), (R, 3)))]
        if R > 0:
            _lib.check(_lib.load().sn_loss_normals_forward(_lib.ptr(weights), _lib.ptr(normals), _lib.ptr(pred_normals), _lib.ptr(directions), R, S,
                                                           *[_lib.ptr(o) for o in outs], _lib.current_stream()), None, "sn_loss_normals_forward")
    return outs


class _NormalTerms(torch.autograd.Function):
    """(weights [R,S], normals [R,S,3], pred_normals [R,S,3], directions [R,3]) -> orientation [R], pred_normal [R], rendered normals
    [R,3], rendered pred_normals [R,3]; only pred_normal is differentiable, and only in pred_normals."""

    @staticmethod
    def forward(ctx, weights, normals, pred_normals, directions):
        ctx.save_for_backward(weights, normals)
        orientation, pred, rn, rpn = _forward(weights, normals, pred_normals, directions, (True, True, True, True))
        ctx.mark_non_differentiable(orientation, rn, rpn)
        return orientation, pred, rn, rpn

    @staticmethod
    @once_differentiable
    def backward(ctx, _g_orientation, g_pred, _g_rn, _g_rpn):
        weights, normals = ctx.saved_tensors
        if g_pred is None or not ctx.needs_input_grad[2]:
            return None, None, None, None
        R, S = weights.shape
        g_pred = g_pred.to(torch.float32).contiguous()
        with torch.cuda.device(weights.device):
            g = torch.empty((R, S, 3), dtype=torch.float32, device=weights.device)
            if R > 0:
                _lib.check(_lib.load().sn_loss_normals_backward(_lib.ptr(weights), _lib.ptr(normals), _lib.ptr(g_pred), R, S, _lib.ptr(g),
                                                                _lib.current_stream()), None, "sn_loss_normals_backward")
        return None, None, g, None


def _check_rays(weights, normals, pred_normals, directions, who: str):
    named = [(weights, "weights"), (normals, "normals")] + ([(pred_normals, "pred_normals")] if pred_normals is not None else []) + \
            ([(directions, "directions")] if directions is not None else [])
    for x, name in named:   # every dtype before any device
        _lib.typed(x, name, mlp.TAKES)
    named = [(_lib.prep(x, name, mlp.TAKES), name) for x, name in named]
    weights, normals = named[0][0], named[1][0]
    pred_normals = named[2][0] if pred_normals is not None else None
    directions = named[-1][0] if directions is not None else None
    if weights.ndim < 2 or weights.shape[-1] != 1:
        raise ValueError(f"{who}: weights [..., S, 1] expected, got {tuple(weights.shape)}")
    lead, S = weights.shape[:-2], weights.shape[-2]
    if not 1 <= S <= 1024:
        raise ValueError(f"{who}: 1..1024 samples per ray expected, got {S}")
    for x, name in ((normals, "normals"), (pred_normals, "pred_normals")):
        if x is not None and x.shape != (*lead, S, 3):
            raise ValueError(f"{who}: {name} {(*lead, S, 3)} expected beside weights {tuple(weights.shape)}, got {tuple(x.shape)}")
    if directions is not None and directions.shape != (*lead, 3):
        raise ValueError(f"{who}: directions {(*lead, 3)} expected beside weights {tuple(weights.shape)}, got {tuple(directions.shape)}")
    for x in (normals, pred_normals, directions):
        if x is not None and x.device != weights.device:
            raise ValueError(f"{who}: every tensor on one device expected, got {weights.device} and {x.device}")
    return weights, normals, pred_normals, directions, lead, S


def _normal_terms(weights: Tensor, normals: Tensor, pred_normals: Tensor, directions: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """All four per-ray terms from one pass over the samples: weights [..., S, 1], normals and pred_normals [..., S, 3], the rays'
    directions [..., 3] -> (orientation [...], pred_normal [...], rendered normals [..., 3], rendered pred_normals [..., 3]).
    ``pred_normal`` is differentiable once in ``pred_normals``; nothing else carries a gradient (the weights and the analytic normals are
    detached in nerfacto's call, and the shaded normals are not read by any loss)."""
    for x, name in ((weights, "weights"), (normals, "normals"), (pred_normals, "pred_normals"), (directions, "directions")):
        _lib.typed(x, name, mlp.TAKES)
    weights, normals, pred_normals, directions, lead, S = _check_rays(weights, normals, pred_normals, directions, "_normal_terms")
    orientation, pred, rn, rpn = _NormalTerms.apply(weights.detach().reshape(-1, S), normals.detach().reshape(-1, S, 3),
                                                    pred_normals.reshape(-1, S, 3), directions.detach().reshape(-1, 3))
    return orientation.reshape(lead), pred.reshape(lead), rn.reshape(*lead, 3), rpn.reshape(*lead, 3)


def normal_losses(weights: Tensor, normals: Tensor, pred_normals: Tensor, directions: Tensor) -> Tuple[Tensor, Tensor]:
    """nerfstudio's ``orientation_loss`` and ``pred_normal_loss`` per ray: (``sum_s w fmin(0, n . (-d))**2``, ``sum_s w (1 - n . n_pred)``),
    each [...].  Shapes and gradients as ``_normal_terms``: differentiable once, in ``pred_normals`` only."""
    orientation, pred, _, _ = _normal_terms(weights, normals, pred_normals, directions)
    return orientation, pred


def render_normals(weights: Tensor, normals: Tensor) -> Tensor:
    """``NormalsRenderer`` + ``NormalsShader``: weights [..., S, 1], normals [..., S, 3] -> ``(v / (|v| + 1e-10) + 1) / 2`` [..., 3] with
    ``v = sum_s w n``.  No gradient."""
    weights, normals, _, _, lead, S = _check_rays(weights, normals, None, None, "render_normals")
    _, _, rn, _ = _forward(weights.detach().reshape(-1, S), normals.detach().reshape(-1, S, 3), None, None, (False, False, True, False))
    return rn.reshape(*lead, 3)
