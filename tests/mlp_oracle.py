"""The trainable MLP as plain torch ops (include/signerf_hip_mlp.h; DESIGN.md §4 "Trainable MLP"), generic in dtype: the forward pass,
the four gradients BY FORMULA (what csrc/sn_mlp.h implements -- tests/test_mlp_host.py holds them against torch.autograd in fp64), the
data of the exact-integer cases with their validity condition, and the gate helper."""
import math

import torch

REAL_STACKS = [(10, 16, 1), (32, 64, 16), (63, 64, 64, 3), (27, 64, 64, 64)]
EDGE_STACKS = [(1, 1), (5, 7, 3), (64, 64, 64, 64, 64), (17, 33, 2)]
STACKS = REAL_STACKS + EDGE_STACKS
# 63 / 64 / 65: the backward kernel's workgroup tile of 64 points and its neighbours; 15 / 16 / 17: a wave's 16 points
SIZES = [1, 15, 16, 17, 63, 64, 65, 1000]
# A backward call has min(ceil(N / 64), 256) workgroups, so a workgroup walks more than one tile of 64 points only above 16384 points:
# 16384 -+ 1 (the last sizes with one tile each; then a second trip for workgroup 0 alone, with one point in it) and 2 * 16384 + 65
# (514 tiles: two trips for every workgroup, a third full tile for workgroup 0 and a third with one point for workgroup 1).
LARGE_SIZES = [16383, 16384, 16385, 2 * 16384 + 65]
# The project's rule for exact-fp32 outputs: e_hip <= F e_ref32 + 1 ulp of the largest output, F = 2, on every output at
# every N >= 16.  Below 16 points y and dW alone are held to F = 8, the widest §5 uses (DESIGN.md §4 "Trainable MLP", "Gates"): there
# e_ref32 is the largest of a handful of draws (ONE draw for the one output of the proposal stack at N = 1), and the kernel's dot product is
# one sequential chain of up to K = 64 fmaf where a CPU GEMM typically adds 8 vector lanes of K / 8 terms each -- the classical bounds of
# those two orders differ by K / (K / 8 + 3) = 5.8 at K = 64.  That is a ratio of BOUNDS; the reference's actual order was not measured.
GATE_FACTOR, SMALL_N_FACTOR = 2.0, {"y": 8.0, "dx": 2.0, "dW": 8.0, "db": 2.0}


def gate_factor(name, N):
    return SMALL_N_FACTOR[name] if N < 16 else GATE_FACTOR


def forward(x, weights, biases, dtype):
    """-> (y [N, d_n], [h_0 .. h_{n-1}]) in dtype: h_0 = x, z_i = h_{i-1} W_i^T + b_i, h_i = relu(z_i), y = z_n."""
    h = x.to(dtype)
    hs = []
    for i, (w, b) in enumerate(zip(weights, biases)):
        hs.append(h)
        h = h @ w.to(dtype).t() + b.to(dtype)
        if i + 1 < len(weights):
            h = torch.relu(h)
    return h, hs


def backward(x, weights, biases, g, dtype):
    """The gradients by formula, last layer first: dZ_n = g; dW_i = dZ_i^T H_{i-1}; db_i = sum_p dZ_i; dH_{i-1} = dZ_i W_i;
    dZ_{i-1} = dH_{i-1} where not (h_{i-1} <= 0), else 0 -- torch's threshold_backward on the relu's RESULT, which lets the gradient of a
    NaN activation pass.  -> (dx, [dW_i], [db_i]) in dtype."""
    _, hs = forward(x, weights, biases, dtype)
    dz = g.to(dtype)
    dws, dbs = [None] * len(weights), [None] * len(weights)
    for i in reversed(range(len(weights))):
        dws[i] = dz.t() @ hs[i]
        dbs[i] = dz.sum(0)
        dh = dz @ weights[i].to(dtype)
        dz = torch.where(hs[i] <= 0, torch.zeros_like(dh), dh) if i > 0 else dh
    return dz, dws, dbs


def autograd(x, weights, biases, g, dtype):
    """The same five through torch.autograd -> (y, dx, [dW_i], [db_i])."""
    xs = x.to(dtype).clone().requires_grad_()
    ws = [w.to(dtype).clone().requires_grad_() for w in weights]
    bs = [b.to(dtype).clone().requires_grad_() for b in biases]
    h = xs
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = torch.nn.functional.linear(h, w, b)
        if i + 1 < len(ws):
            h = torch.relu(h)
    grads = torch.autograd.grad(h, [xs] + ws + bs, g.to(dtype))
    return h.detach(), grads[0], list(grads[1:1 + len(ws)]), list(grads[1 + len(ws):])


def sum_abs_terms(x, weights, biases, g):
    """The largest sum of |terms| over every sum the five outputs are made of, in fp64 (the bias is a term of its layer's sum).  Below 2^24
    with integer operands, every partial sum of every ordering is an integer below 2^24: exact in fp32 in ANY order."""
    D = torch.float64
    _, hs = forward(x, weights, biases, D)
    top = 0.0
    for i, (w, b) in enumerate(zip(weights, biases)):
        top = max(top, float((hs[i].abs() @ w.to(D).abs().t() + b.to(D).abs()).max()))
    dz = g.to(D)
    for i in reversed(range(len(weights))):
        top = max(top, float((dz.abs().t() @ hs[i].abs()).max()), float(dz.abs().sum(0).max()), float((dz.abs() @ weights[i].to(D).abs()).max()))
        dh = dz @ weights[i].to(D)
        dz = torch.where(hs[i] <= 0, torch.zeros_like(dh), dh) if i > 0 else dh
    return top


def integer_case(dims, N, seed=0):
    """x in [-2, 2], W in {-1, 0, 1} with about half its entries zeroed by an independent mask (so W is not symmetric in any sense a
    transposed or permuted operand would survive), b in [-2, 2], g in {-1, 0, 1}: small integers as fp32 -> (x, weights, biases, g)."""
    gen = torch.Generator().manual_seed(1000 * seed + 31 * N + sum((i + 1) * d for i, d in enumerate(dims)))

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)

    x = ints((N, dims[0]), -2, 2)
    weights = [ints((dims[i + 1], dims[i]), -1, 1) * ints((dims[i + 1], dims[i]), 0, 1) for i in range(len(dims) - 1)]
    biases = [ints((dims[i + 1],), -2, 2) for i in range(len(dims) - 1)]
    return x, weights, biases, ints((N, dims[-1]), -1, 1)


def assert_integer_case_is_valid(x, weights, biases, g):
    top = sum_abs_terms(x, weights, biases, g)
    assert top < 2.0**24, f"sum |terms| = {top:.4g} reaches 2^24: the case is not exact in fp32 in every order"
    return top


def linear_init(dims, seed, scale=None):
    """nn.Linear's init, U(-1/sqrt(in), 1/sqrt(in)) for weight and bias, or U(-scale, scale)."""
    gen = torch.Generator().manual_seed(seed)
    weights, biases = [], []
    for i in range(len(dims) - 1):
        k = scale if scale is not None else 1.0 / math.sqrt(dims[i])
        weights.append((torch.rand((dims[i + 1], dims[i]), generator=gen) * 2 - 1) * k)
        biases.append((torch.rand((dims[i + 1],), generator=gen) * 2 - 1) * k)
    return weights, biases


def inputs(dims, N, seed, kind):
    """"uniform": U(-1, 1).  "encoding": the scale of the fields' real inputs -- hash features of about 1e-3 on half the columns (what a
    freshly initialised grid hands over), values in [0, 1] on the others (SH components, an appearance embedding)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand((N, dims[0]), generator=gen) * 2 - 1
    if kind == "encoding":
        x[:, 0::2] *= 1e-3
        x[:, 1::2] = x[:, 1::2].abs()
    g = torch.randn((N, dims[-1]), generator=gen)
    return x, g


def gate(got, ref64, ref32, factor):
    """e_hip <= factor x e_ref32 + 1 ulp of the largest output, e = max |. - ref64| -> (ok, e_hip, e_ref32, the limit, the ratio
    (e_hip - ulp) / e_ref32 the case needs)."""
    e_hip = float((got.double().cpu() - ref64).abs().max())
    e_ref = float((ref32.double() - ref64).abs().max())
    top = float(ref64.abs().max())
    ulp = 2.0 ** (math.frexp(top)[1] - 24) if top > 0 else 2.0**-149
    limit = factor * e_ref + ulp
    need = max(e_hip - ulp, 0.0) / e_ref if e_ref > 0 else (0.0 if e_hip <= ulp else float("inf"))
    return e_hip <= limit, e_hip, e_ref, limit, need
