"""The trainable hash grid as plain torch ops (include/signerf_hip_hashgrid.h; DESIGN.md §4 "Trainable hash grid").  Indices and offsets
come from ``oracle.nerfacto.hash_corner_indices`` in fp32, as the kernels must compute them; the blend (nerfstudio's nesting, as
``oracle.nerfacto.hash_encode`` has it) and its autograd run in a given dtype.  Beside the autograd route the hand-derived formulas the
kernels implement, and per table element the number of contributions ``n`` and ``A = sum w |grad_enc|`` in fp64 that the error bound of
``grad_table`` is made of."""
import torch

from helpers import onf

CORNERS = ("ccc", "cfc", "ffc", "fcc", "ccf", "cff", "fff", "fcf")     # nerfstudio's hashed_0..7: ceil / floor on x y z


def cells(q, scalings, log2_T):
    """q [N,3] fp32, scalings [L] fp32 -> (idx [N,L,8] int64, offset [N,L,3] fp32), oracle.nerfacto's."""
    assert q.dtype == torch.float32 and scalings.dtype == torch.float32
    _, _, idx, offset = onf.hash_corner_indices(q, scalings, log2_T)
    return idx, offset


def blend(f, o):
    """f: the 8 corner rows [N,L,F] each, o [N,L,3] -> [N,L,F], in the nesting of oracle.nerfacto.hash_encode."""
    ox, oy, oz = o[..., 0:1], o[..., 1:2], o[..., 2:3]
    f_03 = f[0] * ox + f[3] * (1 - ox)
    f_12 = f[1] * ox + f[2] * (1 - ox)
    f_56 = f[5] * ox + f[6] * (1 - ox)
    f_47 = f[4] * ox + f[7] * (1 - ox)
    f0312 = f_03 * oy + f_12 * (1 - oy)
    f4756 = f_47 * oy + f_56 * (1 - oy)
    return f0312 * oz + f4756 * (1 - oz)


def gather(table, idx):
    return [table.index_select(0, idx[..., k].reshape(-1)).view(*idx.shape[:-1], table.shape[-1]) for k in range(8)]


def encode(q, table, scalings, log2_T, dtype):
    """-> (enc [N, L*F] in dtype, idx [N,L,8] int64)."""
    idx, offset = cells(q, scalings, log2_T)
    enc = blend(gather(table.to(dtype), idx), offset.to(dtype))
    return enc.flatten(-2, -1), idx


def grads(q, table, scalings, log2_T, grad_enc, dtype):
    """Autograd of the blend in dtype -> (grad_table [L*T,F], grad_q [N,3]).  q enters through the offsets alone (floor has no slope):
    grad_q = sum_l scalings[l] grad_offset[:, l], the chain rule autograd applies to scaled = q * scalings."""
    idx, offset = cells(q, scalings, log2_T)
    t = table.to(dtype).clone().requires_grad_()
    o = offset.to(dtype).clone().requires_grad_()
    enc = blend(gather(t, idx), o).flatten(-2, -1)
    g_t, g_o = torch.autograd.grad(enc, [t, o], grad_enc.to(dtype))
    return g_t, (g_o * scalings.to(dtype).view(1, -1, 1)).sum(1)


def corner_weights(o):
    """o [N,L,3] -> w [N,L,8]: the product of o (ceil) or 1 - o (floor) per axis."""
    return torch.stack([torch.stack([o[..., a] if c[a] == "c" else 1 - o[..., a] for a in range(3)], -1).prod(-1) for c in CORNERS], -1)


def grad_table_formula(idx, offset, grad_enc, rows):
    """d enc / d table[row_k] = wx wy wz: grad_table[row_k] += w_k grad_enc, in grad_enc's dtype."""
    N, L, _ = idx.shape
    w = corner_weights(offset.to(grad_enc.dtype))                                        # [N,L,8]
    g = grad_enc.view(N, L, 1, -1)
    out = torch.zeros(rows, g.shape[-1], dtype=grad_enc.dtype)
    return out.index_add_(0, idx.reshape(-1), (w[..., None] * g).reshape(N * L * 8, -1))


def grad_q_formula(f, offset, scalings, grad_enc):
    """The literal derivative of the blend in the offsets, times the level's scale, summed over features and levels."""
    N, L, _ = offset.shape
    g = grad_enc.view(N, L, -1)
    o = offset.to(g.dtype)
    ox, oy, oz = o[..., 0:1], o[..., 1:2], o[..., 2:3]
    f_03, f_12 = f[0] * ox + f[3] * (1 - ox), f[1] * ox + f[2] * (1 - ox)
    f_56, f_47 = f[5] * ox + f[6] * (1 - ox), f[4] * ox + f[7] * (1 - ox)
    dx = ((f[0] - f[3]) * oy + (f[1] - f[2]) * (1 - oy)) * oz + ((f[4] - f[7]) * oy + (f[5] - f[6]) * (1 - oy)) * (1 - oz)
    dy = (f_03 - f_12) * oz + (f_47 - f_56) * (1 - oz)
    dz = (f_03 * oy + f_12 * (1 - oy)) - (f_47 * oy + f_56 * (1 - oy))
    d = torch.stack([(g * dx).sum(-1), (g * dy).sum(-1), (g * dz).sum(-1)], -1)         # [N,L,3]
    return (d * scalings.to(g.dtype).view(1, -1, 1)).sum(1)


def contributions(idx, offset, grad_enc, rows):
    """Per table element: n, the number of contributions, and A = sum w |grad_enc| in fp64 -> (n [rows,F] int64, A [rows,F] fp64)."""
    N, L, _ = idx.shape
    F = grad_enc.numel() // (N * L)
    A = grad_table_formula(idx, offset.double(), grad_enc.double().abs(), rows)
    n = torch.zeros(rows, dtype=torch.int64).index_add_(0, idx.reshape(-1), torch.ones(N * L * 8, dtype=torch.int64))
    return n[:, None].expand(rows, F).contiguous(), A


def grad_table_bound(n, A):
    """|error| <= (n + 4) 2^-24 A: about 4 roundings in a contribution's product, n - 1 additions in any order."""
    return (n.double() + 4) * 2.0**-24 * A


def gate(got, ref64, ref32):
    """The project's gate: e_hip <= 2 e_ref32 + 1 ulp of the largest output.  -> (ok, e_hip, e_ref32, the limit)."""
    e_hip = float((got.double() - ref64).abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    top = float(ref64.abs().max())
    ulp = 2.0 ** (torch.frexp(torch.tensor(top, dtype=torch.float64))[1].item() - 24) if top > 0 else 2.0**-149
    limit = 2 * e_ref + ulp
    return e_hip <= limit, e_hip, e_ref, limit


def table(L, log2_T, F, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((L << log2_T, F), generator=g) * 2 - 1) * scale


def points(N, seed, lo=0.0, hi=1.0, special=True):
    """U(lo, hi) points; the first rows are replaced by lattice vertices, 0 and nextafter(1, 0) (as many as fit into N - 1 rows)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.rand((N, 3), generator=g) * (hi - lo) + lo
    if special:
        below_one = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
        rows = torch.tensor([[0.25, 0.5, 0.75], [0.0, 0.0, 0.0], [below_one] * 3, [0.5, 0.3, 0.0], [0.1, 0.75, below_one], [0.5, 0.5, 0.5]])
        k = min(len(rows), max(N - 1, 0))
        q[:k] = rows[:k]
    return q
