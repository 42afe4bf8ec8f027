"""The trainable tiny-cuda-nn grid as plain torch ops (signerf_amd/include/signerf_hip_hashgrid_tcnn.h; DESIGN.md §4 "Trainable tcnn grid") on the
UNIFORM table [L * T, F] signerf_amd/tcnn_import.py produces.  Positions, corner rows and weights always come from the fp32
``x = fma(s, q, 0.5)`` and ``oracle.tcnn_layout.grid_rows``, as the kernels must compute them; the blend (``oracle.tcnn_layout.grid_encode``'s
order: weight = ((1 wx) wy) wz, corners summed from 0 up) and its autograd run in a given dtype.  Beside the autograd route: the
hand-derived gradient formulas, and per table element the number of contributions ``n`` and ``A = sum w |grad_enc|`` in fp64 that the error
bound of ``grad_table`` is made of (``hashgrid_oracle.grad_table_bound`` / ``gate`` are shared with the torch-path grid)."""
import torch

import hashgrid_oracle as ho
from oracle import tcnn_layout as tl

SLOT = (7, 5, 4, 6, 3, 1, 0, 2)     # nerfstudio's corner i (hashgrid_oracle.CORNERS, c = + 1) is corner SLOT[i] in bit order


def scalings(meta):
    return torch.tensor(meta.scales, dtype=torch.float32)


def level_rows(meta):
    return [meta.offsets[l + 1] - meta.offsets[l] for l in range(meta.num_levels)]


def uniform_table(flat_rows, meta):
    """Rows back to back [n_rows, F] (the library's layout, what grid_encode reads) -> the uniform [L * T, F] table; unused rows are 0."""
    T = 1 << meta.log2_hashmap_size
    out = torch.zeros((meta.num_levels * T, flat_rows.shape[1]), dtype=flat_rows.dtype)
    for l in range(meta.num_levels):
        out[l * T:l * T + meta.offsets[l + 1] - meta.offsets[l]] = flat_rows[meta.offsets[l]:meta.offsets[l + 1]]
    return out


def flat_rows(table, meta):
    T = 1 << meta.log2_hashmap_size
    return torch.cat([table[l * T:l * T + meta.offsets[l + 1] - meta.offsets[l]] for l in range(meta.num_levels)])


def used_rows(meta):
    """bool [L * T]: the rows of the uniform table some level can address."""
    T = 1 << meta.log2_hashmap_size
    used = torch.zeros(meta.num_levels * T, dtype=torch.bool)
    for l, n in enumerate(level_rows(meta)):
        used[l * T:l * T + n] = True
    return used


def cells(q, meta):
    """q [N,3] fp32 -> (idx [N,L,8] int64 with the level's offset l T, corner k adds 1 on axis a where bit a of k is set;
    w [N,L,3] fp32; x [N,L,3] fp32)."""
    assert q.dtype == torch.float32
    T = 1 << meta.log2_hashmap_size
    idx, ws, xs = [], [], []
    for l in range(meta.num_levels):
        s = torch.tensor(meta.scales[l], dtype=torch.float32)
        x = (q.double() * s.double() + 0.5).float()          # fmaf(s, q, 0.5): the fp64 product of two fp32 is exact, one rounding
        fl = torch.floor(x)
        base = fl.to(torch.int64)
        rows = [tl.grid_rows(meta, l, base + torch.tensor([k & 1, (k >> 1) & 1, (k >> 2) & 1])) + l * T for k in range(8)]
        idx.append(torch.stack(rows, -1))
        ws.append(x - fl)
        xs.append(x)
    return torch.stack(idx, 1), torch.stack(ws, 1), torch.stack(xs, 1)


def in_domain(q, meta):
    """bool [N]: every x finite and in [0, 2^30)."""
    x = cells(q, meta)[2]
    return ((x >= 0) & (x < 2.0**30)).all(-1).all(-1)


def corner_weights(w):
    """w [N,L,3] -> [N,L,8] in w's dtype, in grid_encode's order of operations."""
    out = []
    for k in range(8):
        weight = torch.ones_like(w[..., 0])
        for d in range(3):
            weight = weight * (w[..., d] if k & (1 << d) else 1 - w[..., d])
        out.append(weight)
    return torch.stack(out, -1)


def blend(f, w):
    """f: the 8 corner rows [N,L,F] each, w [N,L,3] -> [N,L,F]: acc = 0; acc = acc + weight_k f_k for k = 0..7."""
    cw = corner_weights(w)
    acc = torch.zeros_like(f[0])
    for k in range(8):
        acc = acc + cw[..., k:k + 1] * f[k]
    return acc


def encode(q, table, meta, dtype):
    """-> (enc [N, L*F] in dtype, idx [N,L,8] int64)."""
    idx, w, _ = cells(q, meta)
    return blend(ho.gather(table.to(dtype), idx), w.to(dtype)).flatten(-2, -1), idx


def grads(q, table, meta, grad_enc, dtype):
    """Autograd of the blend in dtype -> (grad_table [L*T,F], grad_q [N,3]).  q enters through w alone (floor has no slope) and
    d w / d q = s: grad_q = sum_l s_l grad_w[:, l]."""
    idx, w, _ = cells(q, meta)
    t = table.to(dtype).clone().requires_grad_()
    o = w.to(dtype).clone().requires_grad_()
    enc = blend(ho.gather(t, idx), o).flatten(-2, -1)
    g_t, g_o = torch.autograd.grad(enc, [t, o], grad_enc.to(dtype))
    return g_t, (g_o * scalings(meta).to(dtype).view(1, -1, 1)).sum(1)


def grad_table_formula(idx, w, grad_enc, rows):
    """grad_table[row_k] += weight_k grad_enc, in grad_enc's dtype."""
    N, L, _ = idx.shape
    cw = corner_weights(w.to(grad_enc.dtype))
    g = grad_enc.view(N, L, 1, -1)
    out = torch.zeros(rows, g.shape[-1], dtype=grad_enc.dtype)
    return out.index_add_(0, idx.reshape(-1), (cw[..., None] * g).reshape(N * L * 8, -1))


def grad_q_formula(f, w, meta, grad_enc):
    """What the input-gradient kernel evaluates: the torch-path grid's derivative of the trilinear blend (hashgrid_oracle.grad_q_formula)
    on the corners taken in nerfstudio's order, f[SLOT[i]], with w as the weight of the + 1 corners."""
    return ho.grad_q_formula([f[SLOT[i]] for i in range(8)], w, scalings(meta), grad_enc)


def contributions(idx, w, grad_enc, rows):
    """Per table element: n, the number of contributions, and A = sum w |grad_enc| in fp64 -> (n [rows,F] int64, A [rows,F] fp64)."""
    N, L, _ = idx.shape
    F = grad_enc.numel() // (N * L)
    A = grad_table_formula(idx, w.double(), grad_enc.double().abs(), rows)
    n = torch.zeros(rows, dtype=torch.int64).index_add_(0, idx.reshape(-1), torch.ones(N * L * 8, dtype=torch.int64))
    return n[:, None].expand(rows, F).contiguous(), A


def table(meta, F, seed, scale=1.0):
    """A uniform table whose used rows are U(-scale, scale) and whose unused rows are 0, as tcnn_import leaves them."""
    t = ho.table(meta.num_levels, meta.log2_hashmap_size, F, seed, scale)
    return t * used_rows(meta)[:, None]


def points(N, seed, meta=None):
    """U[0, 1) points; the first rows are replaced by rows exactly at 0, at nextafter(1, 0) and at 1.0 (the far-face wrap of the dense
    levels), and -- given the level table -- by rows on lattice planes of the coarsest level (w = 0 there), as many as fit into N - 1."""
    g = torch.Generator().manual_seed(seed)
    q = torch.rand((N, 3), generator=g)
    below_one = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
    rows = [[0.0, 0.0, 0.0], [below_one] * 3, [1.0, 1.0, 1.0], [1.0, 0.3, below_one], [0.0, 1.0, 0.5]]
    if meta is not None:
        s0 = meta.scales[0]
        rows += [[0.5 / s0, 0.3, 0.7], [1.5 / s0, 0.5 / s0, 0.61], [0.5 / s0] * 3]      # x = s q + 0.5 lands on an integer (to a rounding)
    rows = torch.tensor(rows, dtype=torch.float32)
    k = min(len(rows), max(N - 1, 0))
    q[:k] = rows[:k]
    return q


def ray_points(N, seed, per_ray=200):
    """Consecutive samples of a few rays through the unit cube: neighbours share cells on the coarse (dense) levels."""
    g = torch.Generator().manual_seed(seed)
    rays = (N + per_ray - 1) // per_ray
    a, b = torch.rand(rays, 1, 3, generator=g), torch.rand(rays, 1, 3, generator=g)
    t = torch.linspace(0.0, 1.0, per_ray).view(1, per_ray, 1) * 0.999
    return (a + (b - a) * t).reshape(-1, 3)[:N].contiguous()
