"""The normals half of a training step as plain torch ops, generic in dtype (include/signerf_hip_train_normals.h,
include/signerf_hip_normal_losses.h; DESIGN.md §4 "Training-mode normals"): the analytic normal of a point of ``mlp(hash_encode(q))``,
nerfstudio's two normal losses and the rendered normals.  Run in fp64 it is the reference of the tests, run in fp32 the yardstick of their
gate.  A helper, not a test.

Built from the two oracles the kernels' parts already have: tests/hashgrid_oracle.py (``cells`` -- decided in fp32, so that fp64 and the
kernel agree on the voxel --, ``gather``, ``blend``, ``grad_q_formula``) and tests/mlp_oracle.py (``forward`` / ``backward``).  The gate is
tests/normals_oracle.gate with that module's factor, as the eval normals tests use it: e_hip <= GATE_FACTOR x e_ref32 + 1 ulp of the
largest output, e = max |. - ref64|, e_ref32 the fp32 restatement's own error."""
import torch

import hashgrid_oracle as ho
import mlp_oracle as mo
import normals_oracle as no

GATE_FACTOR = no.GATE_FACTOR
ILL_REL = 1e-6          # a row whose fp64 |g| is below this share of its sum of |terms| has no determined direction
MAX_EXCLUDED = 0.02     # at most this share of the rows may be left out of the comparison of normals (never of grad_q)
TIE_REL = 1e-6          # a hidden pre-activation below this share of its own sum of |terms| is a ReLU tie: the seeds have none
STACKS = {16: (32, 64, 16), 5: (10, 16, 1)}      # L -> the stack behind an F = 2 grid of L levels: the main field's, a proposal net's
LOG2_T, F, N_POINTS = 10, 2, 1000
SEEDS = {16: 11, 5: 12}


def analytic(q, table, scalings, log2_T, weights, biases, dtype=torch.float64):
    """Field.get_normals by formula: g_enc = the gradient of output channel 0 of the stack in its input (mlp_oracle.backward of the one-hot),
    g = sum_l s_l sum_f g_enc d blend / d offset (hashgrid_oracle.grad_q_formula), n = -g / max(|g|, 1e-12).  -> dict(g, n [N,3],
    terms [N]: the norm over the axes of sum_l s_l sum_f |g_enc slope|, z: the hidden pre-activations' tie measure [N]) in dtype."""
    assert q.dtype == torch.float32
    idx, offset = ho.cells(q, scalings, log2_T)
    f = ho.gather(table.to(dtype), idx)
    enc = ho.blend(f, offset.to(dtype)).flatten(-2, -1)
    N = q.shape[0]
    one_hot = torch.zeros(N, weights[-1].shape[0], dtype=dtype)
    one_hot[:, 0] = 1
    g_enc, _, _ = mo.backward(enc, weights, biases, one_hot, dtype)
    g = ho.grad_q_formula(f, offset, scalings, g_enc)
    dx, dy, dz = no.level_slopes(f, offset.to(dtype))
    ge = g_enc.view(N, offset.shape[1], -1).abs()
    s = scalings.to(dtype).view(1, -1)
    terms = torch.stack([((ge * d.abs()).sum(-1) * s).sum(-1) for d in (dx, dy, dz)], -1).norm(dim=-1)
    # ReLU ties: |z| of every hidden unit against the sum of |terms| it is made of
    h, tie = enc, torch.full((N,), float("inf"), dtype=dtype)
    for w, b in list(zip(weights, biases))[:-1]:
        z = h @ w.to(dtype).t() + b.to(dtype)
        scale = h.abs() @ w.to(dtype).abs().t() + b.to(dtype).abs()
        tie = torch.minimum(tie, (z.abs() / scale.clamp_min(1e-300)).min(dim=-1).values)
        h = torch.relu(z)
    return {"g": g, "n": -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12), "terms": terms, "tie": tie}


def determined(ref64):
    """[N] bool: the rows whose direction the fp64 reference determines."""
    return ref64["g"].norm(dim=-1) >= ILL_REL * ref64["terms"]


def case(L, N=N_POINTS, zero_row=False):
    """The committed inputs of one grid: N points of hashgrid_oracle.points over [-0.25, 1.25) -- its lattice planes, 0 and nextafter(1, 0)
    among them, and values outside [0, 1] --, a table of 2^10 rows per level, nerfstudio's scalings, the stack by mlp_oracle.linear_init.
    ``zero_row``: row 0 of the last layer's weights zeroed (a zero gradient everywhere)."""
    from helpers import onf

    seed = SEEDS[L]
    q = ho.points(N, seed, lo=-0.25, hi=1.25)
    table = ho.table(L, LOG2_T, F, seed)
    scalings = onf.hash_scalings(L, 16, 2048 if L == 16 else 128)
    weights, biases = mo.linear_init(STACKS[L], seed)
    if zero_row:
        weights[-1][0] = 0.0
    return q, table, scalings, weights, biases


# the other feature counts of the kernel: F = 1 puts four levels into a lane's run of four features (and L F = 8 leaves half a tile empty),
# F = 4 one level, F = 8 half a level (L F = 40: the split crosses a tile boundary, and the last tile is half empty)
FEATURE_CASES = {1: (8, (8, 16, 1)), 4: (6, (24, 32, 4)), 8: (5, (40, 64, 16))}      # F -> (L, stack)
FEATURE_SEEDS = {1: 21, 4: 22, 8: 23}
N_FEATURE_POINTS = 300


def feature_case(F):
    """case() for a grid of F features per level: N_FEATURE_POINTS points, FEATURE_CASES[F] levels up to resolution 512."""
    from helpers import onf

    L, stack = FEATURE_CASES[F]
    seed = FEATURE_SEEDS[F]
    weights, biases = mo.linear_init(stack, seed)
    return ho.points(N_FEATURE_POINTS, seed, lo=-0.25, hi=1.25), ho.table(L, LOG2_T, F, seed), onf.hash_scalings(L, 16, 512), weights, biases


_REFS = {}


def references(L):
    """(inputs, ref64, ref32) of case(L) -- or, for L = ("F", F), of feature_case(F) --, computed once and shared; never modified."""
    if L not in _REFS:
        c = feature_case(L[1]) if isinstance(L, tuple) else case(L)       # ("F", F): the feature-count cases
        _REFS[L] = (c, analytic(*c[:3], LOG2_T, *c[3:], torch.float64), analytic(*c[:3], LOG2_T, *c[3:], torch.float32))
    return _REFS[L]


def gate(got, ref64, ref32, rows=None):
    """normals_oracle.gate on the rows `rows` (all of them by default) -> (ok, e_hip, e_ref32, the limit)."""
    rows = torch.ones(ref64.shape[0], dtype=torch.bool) if rows is None else rows
    return no.gate(got.detach().cpu(), ref64, ref32, rows, GATE_FACTOR)


# ---- the per-ray terms: weights [R,S], normals / pred_normals [R,S,3], directions [R,3] -----------------------------------------------------
def orientation_loss(weights, normals, directions):
    """nerfstudio's orientation_loss: sum_s w fmin(0, n . v)^2 with v = -d."""
    n_dot_v = (normals * (-directions)[:, None, :]).sum(dim=-1)
    return (weights * torch.fmin(torch.zeros_like(n_dot_v), n_dot_v) ** 2).sum(dim=-1)


def pred_normal_loss(weights, normals, pred_normals):
    """nerfstudio's pred_normal_loss: sum_s w (1 - n . n_pred)."""
    return (weights * (1.0 - torch.sum(normals * pred_normals, dim=-1))).sum(dim=-1)


def render_normals(weights, normals):
    """oracle.nerfacto.render_normals: NormalsRenderer (v / (|v| + 1e-10)) and NormalsShader ((v + 1) / 2)."""
    from helpers import onf

    return onf.render_normals(normals, weights[..., None])


def terms(weights, normals, pred_normals, directions, dtype):
    w, n, p, d = (t.to(dtype) for t in (weights, normals, pred_normals, directions))
    return orientation_loss(w, n, d), pred_normal_loss(w, n, p), render_normals(w, n), render_normals(w, p)


def pred_normal_grad(weights, normals, pred_normals, g, dtype):
    """Autograd of pred_normal_loss in pred_normals for the incoming g [R] -> [R,S,3] in dtype."""
    p = pred_normals.to(dtype).clone().requires_grad_()
    (grad,) = torch.autograd.grad(pred_normal_loss(weights.to(dtype), normals.to(dtype), p), p, g.to(dtype))
    return grad


def ray_inputs(R, S, seed):
    """fp32: the weights of loss_oracle.composite_inputs' densities, unit normals and predicted normals, unit directions."""
    import loss_oracle as lo

    deltas, density, _ = lo.composite_inputs(R, S, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    unit = lambda *shape: torch.nn.functional.normalize(torch.randn(*shape, generator=g), dim=-1)  # noqa: E731
    return lo.get_weights(deltas, density).contiguous(), unit(R, S, 3), unit(R, S, 3), unit(R, 3)
