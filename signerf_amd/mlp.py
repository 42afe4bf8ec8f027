"""The trainable MLP: nerfstudio's torch ``MLP`` [NS-RECALL, nerfstudio 1.0.2 ``field_components/mlp.py``; SURVEY.md A8] -- an
``nn.Linear`` stack with a ReLU between layers and no output activation -- as ONE differentiable op in HIP
(include/signerf_hip_mlp.h, csrc/sn_mlp.h) on the weights the ``nn.Linear`` modules hold, ``[out, in]`` row-major, unpacked.

As torch ops every layer is a GEMM, a bias and a ReLU that writes and re-reads an ``[N, width]`` activation, the same again backwards, and
every hidden activation stays alive for autograd.  Here the forward pass keeps nothing but its input, and the backward pass recomputes the
hidden activations of each tile of points (DESIGN.md §4 "Trainable MLP").  The arithmetic is exact fp32 (the f32 matrix instruction) with
``precision="fp32"``, the default, and the method's mixed precision with ``precision="fp16"``: fp16 operands, fp32 accumulation, fp32 master
weights, rounded where include/signerf_hip_mlp.h says (DESIGN.md §4 "Mixed-precision MLP"; csrc/sn_mlp_half.h).  The tensors are fp32 under
both: the kernels round ``x``, the weights and the incoming gradient themselves, and a gradient beyond fp16's range becomes inf there.

Inputs are fp32 GPU tensors: another dtype raises ``TypeError``, a CPU tensor raises ``SignerfHipError`` (there is no CPU path), a
non-contiguous tensor is made contiguous (a contiguous view into the middle of a storage is taken as it is: the entry points ask for 4-byte
alignment only).  1..4 layers, every width in 1..64: the stacks of a default-width nerfacto field; anything else
raises ``ValueError``.  The op is ``once_differentiable``: a second-order request raises instead of being silently wrong.  There are no
float atomics: the output and all gradients are bit-reproducible from call to call.  ``relu(NaN)`` is NaN and the backward mask is
torch's (the gradient passes where the activation is not ``<= 0``).
"""

from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib

MAX_LAYERS, MAX_DIM = _lib.SN_MLP_MAX_LAYERS, _lib.SN_MLP_MAX_DIM
# (the kernels move single fp32 elements: any fp32 tensor's 4-byte alignment is all the entry points ask for)
TAKES = "the MLP kernels take fp32 points and fp32 weights"
PRECISIONS = {"fp32": _lib.SN_MLP_PRECISION_FP32, "fp16": _lib.SN_MLP_PRECISION_FP16}   # SnMlpDesc.precision
WG_POINTS, MAX_PARTIALS = 64, 256   # csrc/sn_mlp.h: the backward kernel's point tile and its cap on partial gradient images


def check_dims(dims: Sequence[int]) -> None:
    """Raises ValueError unless ``dims`` = [in, width..., out] is a stack the kernels take."""
    if not 1 <= len(dims) - 1 <= MAX_LAYERS or not all(1 <= int(d) <= MAX_DIM for d in dims):
        raise ValueError(f"fused_mlp: 1..{MAX_LAYERS} layers with every width in 1..{MAX_DIM} expected, got dims {tuple(dims)} "
                         "(wide, 128-unit fields are not built for the HIP MLP)")


def check_precision(precision) -> int:
    """-> SnMlpDesc.precision; raises ValueError for anything but "fp32" and "fp16"."""
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError(f"fused_mlp: precision={precision!r}: one of {sorted(PRECISIONS)} expected")
    return PRECISIONS[precision]


def partials(N: int) -> int:
    """Partial weight-gradient images of a backward call on N points: a function of N alone."""
    return min((N + WG_POINTS - 1) // WG_POINTS, MAX_PARTIALS)


def workspace_floats(dims: Sequence[int], N: int) -> int:
    """fp32 elements of the backward workspace (``sn_mlp_backward_workspace_bytes`` / 4)."""
    return partials(N) * sum(dims[i + 1] * dims[i] + dims[i + 1] for i in range(len(dims) - 1))


def _desc(dims, weights, biases, grad_weights=None, grad_biases=None, precision: int = 0) -> _lib.SnMlpDesc:
    d = _lib.SnMlpDesc()
    d.n_layers, d.precision = len(weights), precision
    for i, v in enumerate(dims):
        d.dims[i] = v
    for i in range(len(weights)):
        d.weights[i], d.biases[i] = _lib.ptr(weights[i]), _lib.ptr(biases[i])
        if grad_weights is not None:
            d.grad_weights[i], d.grad_biases[i] = _lib.ptr(grad_weights[i]), _lib.ptr(grad_biases[i])
    return d


def _forward(x: Tensor, dims, weights, biases, precision: int = 0) -> Tensor:
    N = x.shape[0]
    with torch.cuda.device(x.device):
        y = torch.empty((N, dims[-1]), dtype=torch.float32, device=x.device)
        if N > 0:
            _lib.check(_lib.load().sn_mlp_forward(C.byref(_desc(dims, weights, biases, precision=precision)), _lib.ptr(x), N, _lib.ptr(y),
                                                  _lib.current_stream()), None, "sn_mlp_forward")
    return y


def _backward(x: Tensor, g: Tensor, dims, weights, biases, want_x: bool, want_w: bool, precision: int = 0):
    """-> (grad_x or None, [grad_W...] or None, [grad_b...] or None); the workspace comes from torch's allocator."""
    N = x.shape[0]
    with torch.cuda.device(x.device):
        g_x = torch.empty_like(x) if want_x else None
        g_w = [torch.empty_like(w) for w in weights] if want_w else None
        g_b = [torch.empty_like(b) for b in biases] if want_w else None
        if N == 0:
            for t in (g_w or []) + (g_b or []):
                t.zero_()
            return g_x, g_w, g_b
        ws = torch.empty(workspace_floats(dims, N), dtype=torch.float32, device=x.device) if want_w else None
        _lib.check(_lib.load().sn_mlp_backward(C.byref(_desc(dims, weights, biases, g_w, g_b, precision)), _lib.ptr(x), _lib.ptr(g), N,
                                               _lib.ptr(g_x), _lib.ptr(ws), 4 * ws.numel() if ws is not None else 0, _lib.current_stream()),
                   None, "sn_mlp_backward")
    return g_x, g_w, g_b


class _FusedMLP(torch.autograd.Function):
    """(precision, x [N, d_0], W_1, b_1, ..., W_n, b_n) -> y [N, d_n]; precision: SnMlpDesc's, not differentiable."""

    @staticmethod
    def forward(ctx, precision, x, *params):
        weights, biases = params[0::2], params[1::2]
        ctx.precision = precision
        ctx.dims = [x.shape[1]] + [w.shape[0] for w in weights]
        ctx.save_for_backward(x, *params)   # the backward pass recomputes the hidden activations from x
        return _forward(x, ctx.dims, weights, biases, precision)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, *params = ctx.saved_tensors
        weights, biases = params[0::2], params[1::2]
        needs = ctx.needs_input_grad[1:]   # (of x and the parameters)
        want_x, want_w = needs[0], any(needs[1:])
        if not (want_x or want_w):
            return (None,) * (2 + len(params))
        g = _lib.prep(g.to(torch.float32), "grad_y", TAKES)
        g_x, g_w, g_b = _backward(x, g, ctx.dims, weights, biases, want_x, want_w, ctx.precision)
        out = [None, g_x]
        for i in range(len(weights)):
            out += [g_w[i] if want_w and needs[1 + 2 * i] else None, g_b[i] if want_w and needs[2 + 2 * i] else None]
        return tuple(out)


def _check(x, weights, biases):
    weights, biases = list(weights), list(biases)
    if len(weights) != len(biases) or not weights:
        raise ValueError(f"fused_mlp: as many weights as biases, at least one, expected; got {len(weights)} and {len(biases)}")
    named = [(x, "x")] + [(w, f"weights[{i}]") for i, w in enumerate(weights)] + [(b, f"biases[{i}]") for i, b in enumerate(biases)]
    for t, name in named:   # every dtype before any device
        _lib.typed(t, name, TAKES)
    x, *rest = [_lib.prep(t, name, TAKES) for t, name in named]
    weights, biases = rest[:len(weights)], rest[len(weights):]
    if x.ndim < 1:
        raise ValueError("fused_mlp: x [..., d_0] expected, got a scalar")
    dims = [x.shape[-1]]
    for i, (w, b) in enumerate(zip(weights, biases)):
        if w.ndim != 2 or w.shape[1] != dims[-1] or b.shape != (w.shape[0],):
            raise ValueError(f"fused_mlp: weights[{i}] [out, {dims[-1]}] and biases[{i}] [out] expected, got {tuple(w.shape)} and {tuple(b.shape)}")
        if w.device != x.device or b.device != x.device:
            raise ValueError(f"fused_mlp: x and every parameter on one device expected, got {x.device}, {w.device}, {b.device}")
        dims.append(w.shape[0])
    check_dims(dims)
    if x.numel() // dims[0] >= 2**31:
        raise ValueError("fused_mlp: fewer than 2**31 points expected")
    return x, weights, biases, dims


def fused_mlp(x: Tensor, weights: Sequence[Tensor], biases: Sequence[Tensor], precision: str = "fp32") -> Tensor:
    """``x [..., d_0]`` through the layers ``weights[i] [d_{i+1}, d_i]``, ``biases[i] [d_{i+1}]`` (an ``nn.Linear``'s ``weight`` and
    ``bias``) with a ReLU between layers and none after the last -> ``[..., d_n]``.  Differentiable once, in ``x`` and in every parameter
    that requires a gradient.  ``precision``: "fp32", exact fp32, or "fp16", fp16 operands with fp32 accumulation (the module docstring)."""
    precision = check_precision(precision)
    x, weights, biases, dims = _check(x, weights, biases)
    lead = x.shape[:-1]
    params = [t for pair in zip(weights, biases) for t in pair]
    y = _FusedMLP.apply(precision, x.reshape(-1, dims[0]), *params)
    return y.reshape(*lead, dims[-1])


def mlp_forward(x: Tensor, weights: Sequence[Tensor], biases: Sequence[Tensor], precision: str = "fp32") -> Tensor:
    """The forward entry point as it is, no autograd graph: for tests and measurements."""
    precision = check_precision(precision)
    x, weights, biases, dims = _check(x, weights, biases)
    return _forward(x.detach().reshape(-1, dims[0]), dims, [w.detach() for w in weights], [b.detach() for b in biases],
                    precision).reshape(*x.shape[:-1], dims[-1])


def mlp_backward(x: Tensor, weights: Sequence[Tensor], biases: Sequence[Tensor], grad_y: Tensor, want_grad_x: bool = True,
                 want_grad_params: bool = True, precision: str = "fp32"):
    """The backward entry point as it is, for tests and measurements -> (grad_x or None, [grad_W...] or None, [grad_b...] or None)."""
    precision = check_precision(precision)
    x, weights, biases, dims = _check(x, weights, biases)
    grad_y = _lib.prep(grad_y, "grad_y", TAKES).detach()
    N = x.numel() // dims[0]
    if grad_y.numel() != N * dims[-1]:
        raise ValueError(f"mlp_backward: grad_y [..., {dims[-1]}] for {N} points expected, got {tuple(grad_y.shape)}")
    if not (want_grad_x or want_grad_params):
        raise ValueError("mlp_backward: want_grad_x or want_grad_params expected")
    g_x, g_w, g_b = _backward(x.detach().reshape(-1, dims[0]), grad_y.reshape(-1, dims[-1]), dims, [w.detach() for w in weights],
                              [b.detach() for b in biases], want_grad_x, want_grad_params, precision)
    return (g_x.reshape(x.shape) if g_x is not None else None), g_w, g_b
