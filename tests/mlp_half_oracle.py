"""The mixed-precision MLP (SnMlpDesc.precision = 1; include/signerf_hip_mlp.h, DESIGN.md §4 "Mixed-precision MLP") as torch ops on the CPU.

``forward`` / ``backward`` with ``dtype=torch.float64`` are the SPECIFICATION: every rounding point of csrc/sn_mlp_half.h -- r16 of x, of the
weights, of every hidden activation, of g and of every hidden gradient -- with the sums between them in fp64.  With ``dtype=torch.float32``
they are the RESTATEMENT: the same rounding points with fp32 accumulation (``perm_seed`` sums in a random order of the terms).  ``bounds``
gives, per element and from the specification's own values, the two bounds the tests hold the kernel and the restatement to, and asserts the
conditions under which they mean something.  ``integer_case`` is the exact data of the layout test, ``random_case`` the random data."""
import math

import numpy as np
import torch

import mlp_oracle as mo

D = torch.float64
U32 = 2.0**-24              # the unit roundoff of fp32
U16 = 2.0**-11              # ... of fp16: a value that lands on the NEIGHBOURING fp16 value moves by 2 U16 = 2^-10 of itself
TINY16 = 2.0**-14           # the smallest normal fp16
# The subnormal question: does the f16 matrix instruction keep subnormal fp16 OPERANDS?  False = they are kept (gradual underflow, IEEE);
# True would make r16 flush everything below 2^-14 to zero, here and in the documentation.
FLUSH_SUBNORMALS = False
# weights: nn.Linear's init scale (None) and 1e-3; inputs: U(-1, 1), 1e-4 U(-1, 1) (the hash features' scale at nerfstudio's init, just
# above fp16's smallest normal: its products and roundings live among the subnormals) and 30 U(-1, 1)
WEIGHT_SCALES = [None, 1e-3]
INPUT_SCALES = [1.0, 1e-4, 30.0]
SIZES = mo.SIZES + [16385, 2 * 16384 + 65]
# non-zero share of the {-1, 0, 1} weights of the integer cases.  One value serves every stack of mlp_oracle.STACKS: at it the largest
# rounded value over all stacks and sizes is 959 (limit 2048: integers up to there are exact in fp16) and the largest sum of |terms|
# 5.9e6 (limit 2^24), both on (64, 64, 64, 64, 64); tests/test_mlp_half_host.py asserts both for every stack and size, and at least 5 %
# non-zeros in every matrix of 256 entries or more
INTEGER_DENSITY = 0.5


def r16(t):
    """Round to nearest even to IEEE fp16 and back, ONCE: overflow gives +-inf, subnormals are kept, NaN stays NaN.  An fp64 tensor goes
    through numpy, whose conversion rounds the double itself; torch's takes it through fp32 first, and that double rounding moves a
    value that lies just beside the midpoint of two fp16 values to the wrong one (about one hidden value in 2^14)."""
    if t.dtype == torch.float64:
        with np.errstate(over="ignore"):
            r = torch.from_numpy(t.numpy().astype(np.float16))
    else:
        r = t.to(torch.float16)
    if FLUSH_SUBNORMALS:
        r = torch.where(r.abs() < TINY16, torch.zeros_like(r) * r, r)
    return r.to(t.dtype)


def _mm(a, b, perm_seed):
    """a @ b; with a seed the terms of every sum are presented to the GEMM in a random order."""
    if perm_seed is None:
        return a @ b
    p = torch.randperm(a.shape[1], generator=torch.Generator().manual_seed(perm_seed))
    return a[:, p].contiguous() @ b[p].contiguous()


def forward(x, weights, biases, dtype, perm_seed=None):
    """-> (y, [h_0 .. h_{n-1}] rounded, [z_1 .. z_n]) in dtype."""
    h = r16(x).to(dtype)
    hs, zs = [], []
    for i, (w, b) in enumerate(zip(weights, biases)):
        hs.append(h)
        z = _mm(h, r16(w).to(dtype).t(), perm_seed) + b.to(dtype)
        zs.append(z)
        h = r16(torch.relu(z)) if i + 1 < len(weights) else z
    return h, hs, zs


def backward(x, weights, biases, g, dtype, perm_seed=None):
    """-> (dx, [dW_i], [db_i], [dZ_1 .. dZ_n] rounded, [dH_0 .. dH_{n-1}]) in dtype."""
    n = len(weights)
    _, hs, _ = forward(x, weights, biases, dtype, perm_seed)
    dz = r16(g).to(dtype)
    dws, dbs, dzs, dhs = [None] * n, [None] * n, [None] * n, [None] * n
    for i in reversed(range(n)):
        dzs[i] = dz
        dws[i] = _mm(dz.t(), hs[i], perm_seed)
        dbs[i] = dz.sum(0)
        dhs[i] = _mm(dz, r16(weights[i]).to(dtype), perm_seed)
        if i > 0:
            dz = torch.where(hs[i] <= 0, torch.zeros_like(dhs[i]), r16(dhs[i]))     # the mask on the ROUNDED activation
    return dhs[0], dws, dbs, dzs, dhs


def outputs(x, weights, biases, g, dtype, perm_seed=None):
    """(y, dx, [dW], [db]) -- the four the kernels return."""
    y = forward(x, weights, biases, dtype, perm_seed)[0]
    dx, dw, db, _, _ = backward(x, weights, biases, g, dtype, perm_seed)
    return y, dx, dw, db


def flat(r):
    """(name, tensor) of every output of a (y, dx, [dW], [db]) result."""
    return [("y", r[0]), ("dx", r[1])] + [(f"dW{i}", t) for i, t in enumerate(r[2])] + [(f"db{i}", t) for i, t in enumerate(r[3])]


def bounds(x, weights, biases, g):
    """-> (spec, tight, flip, info): the specification's outputs in fp64; ``tight`` = {"y", "dx"} -> B_tight; ``flip`` = the same layout as
    ``spec`` -> B_flip; info = figures of the case.  Asserts that every value is finite: no value of a finite case overflows fp16.

    The ReLU mask.  h = r16(relu(z)) is 0 up to z = 2^-25 and 2^-24 just above it; where the kernel's z can lie on the other side of that
    point than this file's, dZ is r16(dH) on one side and 0 on the other, and no bound on roundings covers that.  The elements where it
    can happen are those with z in (0, 2^-24], or with 2^-25 within R_z of z, where R_z is the deviation the kernel's z can REACH:
    R_h0 = 0; R_z = |W| R_h + (K + 2) u32 (|W| |h| + |b|); R_h = R_z, plus 2^-10 max(|z|, 2^-14) only at the elements whose rounding
    r16(relu(.)) differs between z - R_z and z + R_z -- the hidden values that fp32 accumulation can put on the neighbouring fp16 value.
    (B_flip's own E_z lets EVERY hidden value move: as the window it marks about 2 % of the hidden values of the deep stacks and
    widens B_flip of their dW 35 to 60 times.  The accumulation term alone is too narrow: one hidden value on its neighbour moves the next
    layer's z by |W| 2^-10 |h|, and on an MI355X dx of (63, 64, 64, 3), init scale, N = 32833 then reaches 1.28 x B_flip in one row.)
    Such elements cannot be kept out of the cases, so E_dZ gains |dH| at exactly these elements and is the plain recursion everywhere
    else; info["ambiguous"] counts them (over the GPU test's 480 cases 0.026 % of the hidden values, at most 0.29 % of a case's) and
    info["inflation"] is the median, over the elements of dx and every dW and db, of B_flip against the plain recursion (1.00 in most
    cases, at most 1.79).  Forwards nothing is needed: 0 against 2^-24 is inside E_h."""
    n = len(weights)
    y, hs, zs = forward(x, weights, biases, D)
    dx, dws, dbs, dzs, dhs = backward(x, weights, biases, g, D)
    A = [r16(w).to(D).abs() for w in weights]
    for t in [y, dx] + hs + dzs + dhs + dws + dbs:
        assert torch.isfinite(t).all(), "a finite case overflows fp16 somewhere"
    N = x.shape[0]
    # forwards: E_h0 = 0; E_z = |W| E_h + (K + 2) u32 (|W| |h| + |b|); E_h = E_z + 2^-10 max(|z|, 2^-14); beside it R_z, R_h (above)
    e_h, r_h, ambiguous = [torch.zeros_like(hs[0])], torch.zeros_like(hs[0]), [None]
    for i in range(n):
        K = weights[i].shape[1]
        acc = (K + 2) * U32 * (hs[i].abs() @ A[i].t() + biases[i].to(D).abs())
        e_z = e_h[i] @ A[i].t() + acc
        if i + 1 < n:
            step = 2 * U16 * zs[i].abs().clamp_min(TINY16)
            e_h.append(e_z + step)
            r_z = r_h @ A[i].t() + acc
            ambiguous.append(((zs[i] > 0) & (zs[i] <= 2.0**-24)) | ((zs[i] - 2.0**-25).abs() <= r_z))    # (of h_{i+1}, layer i + 1's input)
            r_h = r_z + torch.where(r16(torch.relu(zs[i] - r_z)) != r16(torch.relu(zs[i] + r_z)), step, torch.zeros_like(step))
    tight = {"y": acc}
    flip_y = e_z

    def backwards(mask_allowance):
        """E_dZn = 0; E_dH = E_dZ |W| + (K + 2) u32 |dZ| |W|; E_dZ = E_dH + 2^-10 max(|dH|, 2^-14) (+ |dH| where the mask is ambiguous)"""
        e_dz = torch.zeros_like(dzs[n - 1])
        b_w, b_b = [None] * n, [None] * n
        for i in reversed(range(n)):
            az, ah = dzs[i].abs(), hs[i].abs()
            b_w[i] = e_dz.t() @ ah + az.t() @ e_h[i] + e_dz.t() @ e_h[i] + (N + 2) * U32 * (az.t() @ ah)
            b_b[i] = e_dz.sum(0) + (N + 2) * U32 * az.sum(0)
            acc = (weights[i].shape[0] + 2) * U32 * (az @ A[i])
            e_dh = e_dz @ A[i] + acc
            if i > 0:
                e_dz = e_dh + 2 * U16 * dhs[i].abs().clamp_min(TINY16)
                if mask_allowance:
                    e_dz = e_dz + torch.where(ambiguous[i], dhs[i].abs(), torch.zeros_like(e_dh))
        return acc, e_dh, b_w, b_b

    tight["dx"], flip_x, flip_w, flip_b = backwards(True)
    _, plain_x, plain_w, plain_b = backwards(False)
    ratios = torch.cat([(a / b.clamp_min(1e-300)).flatten() for a, b in zip([flip_x] + flip_w + flip_b, [plain_x] + plain_w + plain_b)])
    info = {"subnormal_hidden": sum(int(((h.abs() > 0) & (h.abs() < TINY16)).sum()) for h in hs),
            "subnormal_grad": sum(int(((t.abs() > 0) & (t.abs() < TINY16)).sum()) for t in dzs),
            "ambiguous": sum(int(a.sum()) for a in ambiguous[1:]), "hidden": sum(a.numel() for a in ambiguous[1:]),
            "inflation": float(ratios.median()), "inflation_max": float(ratios.max()), "largest": max(float(t.abs().max()) for t in hs + dzs)}
    return (y, dx, dws, dbs), tight, (flip_y, flip_x, flip_w, flip_b), info


def rows_above(got, want, bound, factor):
    """Rows of a [N, d] output with any element further than factor x bound from `want`."""
    return int(((got.double() - want).abs() > factor * bound).any(dim=1).sum())


def row_cap(N):
    return max(1, math.ceil(0.05 * N))


# ---- data --------------------------------------------------------------------------------------------------------------------------------
def integer_case(dims, N, seed=0):
    """x in [-2, 2], b in [-2, 2], g in {-1, 0, 1}, W in {-1, 0, 1} under an independent zero mask that keeps INTEGER_DENSITY of the
    entries: small integers as fp32 -> (x, weights, biases, g)."""
    gen = torch.Generator().manual_seed(1000 * seed + 31 * N + sum((i + 1) * d for i, d in enumerate(dims)) + 7)
    keep = INTEGER_DENSITY

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)

    def signs(shape):
        return (ints(shape, 0, 1) * 2 - 1) * (torch.rand(shape, generator=gen) < keep).to(torch.float32)

    x = ints((N, dims[0]), -2, 2)
    weights = [signs((dims[i + 1], dims[i])) for i in range(len(dims) - 1)]
    biases = [ints((dims[i + 1],), -2, 2) for i in range(len(dims) - 1)]
    return x, weights, biases, ints((N, dims[-1]), -1, 1)


def integer_case_figures(x, weights, biases, g):
    """-> (the largest magnitude of any value that is rounded to fp16, the largest sum of |terms| of any sum), in fp64 on the plain
    network (on integer data within these limits nothing rounds, so it IS the specification)."""
    _, hs = mo.forward(x, weights, biases, D)
    dz, top = g.to(D), float(g.abs().max())
    for i in reversed(range(len(weights))):
        top = max(top, float(hs[i].abs().max()), float(dz.abs().max()))
        dh = dz @ weights[i].to(D)
        dz = torch.where(hs[i] <= 0, torch.zeros_like(dh), dh) if i > 0 else dh
    return top, mo.sum_abs_terms(x, weights, biases, g)


def random_case(dims, N, wscale, xscale):
    """-> (x, weights, biases, g): weights U(-k, k) with k = 1 / sqrt(in) or wscale, x = xscale U(-1, 1), g standard normal."""
    w, b = mo.linear_init(dims, seed=11 + len(dims), scale=wscale)
    gen = torch.Generator().manual_seed(5 * N + dims[0] + int(round(math.log10(xscale) * 10)) + 100)
    x = (torch.rand((N, dims[0]), generator=gen) * 2 - 1) * xscale
    g = torch.randn((N, dims[-1]), generator=gen)
    return x, w, b, g
