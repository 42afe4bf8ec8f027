"""The trainable hash grid: nerfstudio's torch-path ``HashEncoding`` [NS-RECALL, nerfstudio 1.0.2 ``field_components/encodings.py``;
SURVEY.md A7] as a differentiable op in HIP (include/signerf_hip_hashgrid.h, csrc/sn_hashgrid.h) on the table a ``nn.Parameter`` holds.

It is the one piece of a nerfacto field that plain torch ops do badly -- every point fetches 8 L rows and the backward pass is an
``index_add`` over 8 L N scattered rows -- and the keystone of a training step: with it ``nerfacto.MLPWithHashEncoding(...)(q)`` is a
differentiable module, and the rest of the field (the ``nn.Linear`` stacks, the SH encoding, ``trunc_exp``, the contraction) runs as torch
ops (DESIGN.md §4 "Trainable hash grid").

Inputs are fp32 GPU tensors: another dtype raises ``TypeError``, a CPU tensor raises ``SignerfHipError`` (there is no CPU path), a
non-contiguous tensor is made contiguous.  What gets a gradient: the table, and ``q`` when it requires one; never the scalings.  The op is
``once_differentiable``: a second-order request (analytic-normal losses) raises instead of being silently wrong.  With the default
``table_grad="atomic"`` ``grad_table`` is summed with fp32 atomics, so two backward passes may differ in its last bits; with
``table_grad="ordered"`` (signerf_amd/include/signerf_hip_hashgrid_ordered.h; DESIGN.md §4 "Ordered table gradient") every contribution is stored,
sorted by row and summed in fp64 in a fixed order, without a float atomic, and two backward passes give the same bits.  The features and
``grad_q`` are bit-reproducible either way.  A point with a
non-finite coordinate, or with ``|q * scaling| >= 2**30`` at any level, gives NaN features and a NaN ``grad_q`` row and adds nothing to
the table's gradient.

``grid="tcnn"`` on the three functions below runs the same kernels on tiny-cuda-nn's grid (signerf_amd/include/signerf_hip_hashgrid_tcnn.h; DESIGN.md §4
"Trainable tcnn grid"): the uniform table ``tcnn_import`` produces, the library's scales, floor / floor + 1 corners in bit order (bit a
of corner k adds 1 on axis a) and densely indexed coarse levels.  There a point is in domain iff ``fma(scaling, q, 0.5)`` is finite and
in ``[0, 2**30)`` on every axis at every level; outside it the behaviour is the one described above.
"""

from __future__ import annotations

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib

FEATURES = (1, 2, 4, 8)
MAX_LEVELS, MAX_LOG2_T = 32, 24
TAKES = "the hash-grid kernels take fp32 points and fp32 tables"
GRIDS = {"torch": "sn_hashgrid", "tcnn": "sn_hashgrid_tcnn"}   # grid -> the prefix of its forward / backward entry points
TABLE_GRADS = ("atomic", "ordered")
ORDERED = {"torch": "sn_hashgrid_ordered_backward", "tcnn": "sn_hashgrid_ordered_tcnn_backward"}


def _entry(grid: str, which: str):
    """(the entry point, its name) of a grid's forward or backward."""
    if grid not in GRIDS:
        raise ValueError(f"grid={grid!r}: one of {sorted(GRIDS)} expected")
    name = f"{GRIDS[grid]}_{which}"
    return getattr(_lib.load(), name), name


def _check_table_grad(table_grad: str) -> None:
    if table_grad not in TABLE_GRADS:
        raise ValueError(f"table_grad={table_grad!r}: one of {TABLE_GRADS} expected")


def _backward(grid: str, table_grad: str, q, table, scalings, g, N, L, log2_T, F, g_table, g_q) -> None:
    """The backward entry point of a grid in the chosen form of the table gradient.  The ordered form's workspace is a uint8 tensor on the
    current device: torch's allocator keeps it alive for the stream it was allocated on."""
    if table_grad == "atomic":
        fn, name = _entry(grid, "backward")
        _lib.check(fn(_lib.ptr(q), _lib.ptr(table), _lib.ptr(scalings), _lib.ptr(g), N, L, log2_T, F, _lib.ptr(g_table), _lib.ptr(g_q),
                      _lib.current_stream()), None, name)
        return
    if grid not in GRIDS:
        raise ValueError(f"grid={grid!r}: one of {sorted(GRIDS)} expected")
    lib, name = _lib.load(), ORDERED[grid]
    size = lib.sn_hashgrid_ordered_workspace_bytes(N, L, log2_T, F) if g_table is not None else 0   # (0: the entry point says why)
    ws = torch.empty(size, dtype=torch.uint8, device=q.device) if size else None
    _lib.check(getattr(lib, name)(_lib.ptr(q), _lib.ptr(table), _lib.ptr(scalings), _lib.ptr(g), N, L, log2_T, F, _lib.ptr(g_table), _lib.ptr(g_q),
                                  _lib.ptr(ws), size, _lib.current_stream()), None, name)


def tcnn_levels(scalings, log2_hashmap_size: int):
    """(res, rows, dense) per level of a tiny-cuda-nn grid as the kernels derive them from its scalings (host only, no device):
    r = ceil(s) + 1, n = min(next_multiple(r**3, 8), T), dense iff r**3 <= n."""
    import ctypes as C

    s = [float(v) for v in scalings]
    L = len(s)
    arr = (C.c_float * max(L, 1))(*s)
    res, rows, dense = ((C.c_int32 * max(L, 1))() for _ in range(3))
    _lib.check(_lib.load().sn_hashgrid_tcnn_levels(arr, L, log2_hashmap_size, res, rows, dense), None, "sn_hashgrid_tcnn_levels")
    return list(res[:L]), list(rows[:L]), [bool(d) for d in dense[:L]]


def _prep(x, name: str) -> Tensor:
    x = _lib.prep(x, name, TAKES)
    return x if x.data_ptr() % 16 == 0 else x.clone(memory_format=torch.contiguous_format)   # (a view into the middle of a storage)


class _HashEncode(torch.autograd.Function):
    """(q [N,3], table [L*T,F], scalings [L], log2_T, grid, table_grad) -> enc [N, L*F]."""

    @staticmethod
    def forward(ctx, q, table, scalings, log2_T, grid="torch", table_grad="atomic"):
        N, L, F = q.shape[0], scalings.shape[0], table.shape[1]
        ctx.save_for_backward(q, table, scalings)   # the backward pass recomputes indices and weights from q
        ctx.log2_T, ctx.grid, ctx.table_grad = log2_T, grid, table_grad
        with torch.cuda.device(q.device):
            enc = torch.empty((N, L * F), dtype=torch.float32, device=q.device)
            if N > 0:
                fn, name = _entry(grid, "forward")
                _lib.check(fn(_lib.ptr(q), _lib.ptr(table), _lib.ptr(scalings), N, L, log2_T, F, _lib.ptr(enc), None, _lib.current_stream()), None, name)
        return enc

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, table, scalings = ctx.saved_tensors
        N, L, F = q.shape[0], scalings.shape[0], table.shape[1]
        want_q, want_table = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_q or want_table):
            return None, None, None, None, None, None
        g = _prep(g.to(torch.float32), "grad_enc")
        with torch.cuda.device(q.device):
            g_table = torch.zeros_like(table) if want_table else None     # accumulated into by ONE backward call
            g_q = torch.empty_like(q) if want_q else None
            if N > 0:
                _backward(ctx.grid, ctx.table_grad, q, table, scalings, g, N, L, ctx.log2_T, F, g_table, g_q)
        return g_q, g_table, None, None, None, None


def _check(q: Tensor, hash_table: Tensor, scalings: Tensor, log2_hashmap_size: int, grid: str = "torch"):
    if grid not in GRIDS:
        raise ValueError(f"hash_encode: grid={grid!r}: one of {sorted(GRIDS)} expected")
    for x, name in ((q, "q"), (hash_table, "hash_table"), (scalings, "scalings")):   # every dtype before any device
        _lib.typed(x, name, TAKES)
    q, hash_table, scalings = _prep(q, "q"), _prep(hash_table, "hash_table"), _prep(scalings, "scalings").detach()
    if q.ndim < 1 or q.shape[-1] != 3:
        raise ValueError(f"hash_encode: q [..., 3] expected, got {tuple(q.shape)}")
    L = scalings.numel()
    if scalings.ndim != 1 or not 1 <= L <= MAX_LEVELS:
        raise ValueError(f"hash_encode: scalings [L] with 1 <= L <= {MAX_LEVELS} expected, got {tuple(scalings.shape)}")
    if not isinstance(log2_hashmap_size, int) or not 1 <= log2_hashmap_size <= MAX_LOG2_T:
        raise ValueError(f"hash_encode: log2_hashmap_size in 1..{MAX_LOG2_T} expected, got {log2_hashmap_size!r}")
    if hash_table.ndim != 2 or hash_table.shape[0] != L << log2_hashmap_size or hash_table.shape[1] not in FEATURES:
        raise ValueError(f"hash_encode: hash_table [L * 2**log2_hashmap_size, F] = [{L << log2_hashmap_size}, F] with F in {FEATURES} "
                         f"expected, got {tuple(hash_table.shape)}")
    if hash_table.numel() >= 2**31:
        raise ValueError(f"hash_encode: a table of {hash_table.numel()} elements: fewer than 2**31 expected (32-bit element offsets)")
    if not (q.device == hash_table.device == scalings.device):
        raise ValueError(f"hash_encode: q, hash_table and scalings on one device expected, got {q.device}, {hash_table.device}, {scalings.device}")
    return q, hash_table, scalings


def hash_encode(q: Tensor, hash_table: Tensor, scalings: Tensor, log2_hashmap_size: int, grid: str = "torch",
                table_grad: str = "atomic") -> Tensor:
    """nerfstudio's ``HashEncoding.pytorch_fwd``: q [..., 3] (the field's positions in [0, 1]), hash_table [L * 2**log2_hashmap_size, F],
    scalings [L] -> [..., L * F], level-major.  Differentiable once, in ``hash_table`` and (when it requires a gradient) in ``q``.
    ``grid="tcnn"``: tiny-cuda-nn's grid on the same uniform table (the module docstring).  ``table_grad``: "atomic" (fp32 atomic adds) or
    "ordered" (the bit-reproducible fp64 sum in a fixed order) for the table's gradient; the features do not depend on it."""
    _check_table_grad(table_grad)
    q, hash_table, scalings = _check(q, hash_table, scalings, log2_hashmap_size, grid)
    lead = q.shape[:-1]
    enc = _HashEncode.apply(q.reshape(-1, 3), hash_table, scalings, log2_hashmap_size, grid, table_grad)
    return enc.reshape(*lead, enc.shape[-1])


def hash_corner_indices(q: Tensor, hash_table: Tensor, scalings: Tensor, log2_hashmap_size: int, grid: str = "torch"):
    """For inspection and tests, no gradient: (enc [..., L * F], idx [..., L, 8] int32), the table row (with its level's offset) of every
    corner in nerfstudio's order hashed_0..7 -- with ``grid="tcnn"`` in that grid's bit order."""
    q, hash_table, scalings = _check(q, hash_table, scalings, log2_hashmap_size, grid)
    q, hash_table = q.detach(), hash_table.detach()
    lead, L, F = q.shape[:-1], scalings.numel(), hash_table.shape[1]
    N = q.numel() // 3
    with torch.cuda.device(q.device):
        enc = torch.empty((*lead, L * F), dtype=torch.float32, device=q.device)
        idx = torch.empty((*lead, L, 8), dtype=torch.int32, device=q.device)
        if N > 0:
            fn, name = _entry(grid, "forward")
            _lib.check(fn(_lib.ptr(q), _lib.ptr(hash_table), _lib.ptr(scalings), N, L, log2_hashmap_size, F, _lib.ptr(enc), _lib.ptr(idx),
                          _lib.current_stream()), None, name)
    return enc, idx


def hash_encode_backward(q: Tensor, hash_table: Tensor, scalings: Tensor, log2_hashmap_size: int, grad_enc: Tensor,
                         grad_table: Tensor = None, want_grad_q: bool = False, grid: str = "torch", table_grad: str = "atomic"):
    """The backward entry point as it is, for tests and measurements: ``grad_table`` (or None) is ACCUMULATED INTO, ``grad_q`` (or None)
    is returned.  -> (grad_table, grad_q).  ``table_grad="ordered"`` calls the ordered entry point of the grid with a workspace of its own."""
    _check_table_grad(table_grad)
    q, hash_table, scalings = _check(q, hash_table, scalings, log2_hashmap_size, grid)
    q, hash_table, grad_enc = q.detach(), hash_table.detach(), _prep(grad_enc, "grad_enc").detach()
    L, F = scalings.numel(), hash_table.shape[1]
    N = q.numel() // 3
    if grad_enc.numel() != N * L * F:
        raise ValueError(f"hash_encode_backward: grad_enc [..., {L * F}] for {N} points expected, got {tuple(grad_enc.shape)}")
    if grad_table is None and not want_grad_q:
        raise ValueError("hash_encode_backward: grad_table or want_grad_q expected")
    if grad_table is not None and (grad_table.shape != hash_table.shape or _prep(grad_table, "grad_table").data_ptr() != grad_table.data_ptr()):
        raise ValueError("hash_encode_backward: grad_table must be a contiguous, 16-byte aligned tensor of the table's shape")
    with torch.cuda.device(q.device):
        grad_q = torch.empty_like(q) if want_grad_q else None
        if N > 0:
            _backward(grid, table_grad, q, hash_table, scalings, grad_enc, N, L, log2_hashmap_size, F, grad_table, grad_q)
    return grad_table, grad_q
