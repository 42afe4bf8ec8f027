"""The analytic normals of training samples on the GPU (signerf_amd/train_normals.py over csrc/sn_train_normals.h) against the fp64
restatement of tests/train_normals_oracle.py: the fused kernel, the composed route (sn_mlp_backward, then sn_hashgrid_backward), their
sign, the zero gradient, reproducibility, the domain rule, the edge sizes and the refusals.

Gate (train_normals_oracle.gate = normals_oracle.gate, factor 8): max |kernel - ref64| <= 8 x max |restatement32 - ref64| + 1 ulp of the
largest output.  ``grad_q`` is compared on every element; ``normals`` on the rows whose direction the reference determines (fp64 |g| at
least 1e-6 of its sum of |terms|; at most 2 % may be left out -- tests/test_train_normals_host.py holds the seeds to that on the CPU).
Every figure is printed before it is asserted (pytest -s shows them)."""
import ctypes as C

import pytest
import torch

import train_normals_oracle as to
from signerf_amd import _lib, mlp, train_normals

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(gpu):
    """A device error ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize(gpu)
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _on(gpu, case):
    q, table, scalings, weights, biases = case
    return q.to(gpu), table.to(gpu), scalings.to(gpu), to.LOG2_T, [w.to(gpu) for w in weights], [b.to(gpu) for b in biases]


def _check(name, normals, grad, ref64, ref32):
    det = to.determined(ref64)
    excluded = int((~det).sum())
    assert excluded <= to.MAX_EXCLUDED * det.numel()
    assert normals.shape == grad.shape == ref64["g"].shape and not normals.requires_grad and not grad.requires_grad
    ok_g, e_g, r_g, lim_g = to.gate(grad, ref64["g"], ref32["g"])
    ok_n, e_n, r_n, lim_n = to.gate(normals, ref64["n"], ref32["n"], det)
    print(f"{name}: grad_q e_hip {e_g:.2e} e_ref32 {r_g:.2e} limit {lim_g:.2e} | normals e_hip {e_n:.2e} e_ref32 {r_n:.2e} limit {lim_n:.2e} "
          f"| {excluded} of {det.numel()} rows left out of the normals")
    assert ok_g, f"{name}: grad_q {e_g:.3e} > {lim_g:.3e}"
    assert ok_n, f"{name}: normals {e_n:.3e} > {lim_n:.3e}"


@pytest.mark.parametrize("L", [16, 5])
def test_fused_kernel_against_fp64(gpu, L):
    case, ref64, ref32 = to.references(L)
    normals, grad = train_normals.analytic_normals(*_on(gpu, case), return_grad=True)
    _check(f"fused L={L} {to.STACKS[L]}", normals, grad, ref64, ref32)
    assert torch.equal(train_normals.analytic_normals(*_on(gpu, case)), normals)      # (without grad_q: the same normals)


@pytest.mark.parametrize("F", [1, 4, 8])
def test_other_feature_counts_against_fp64(gpu, F):
    """F = 1 (four levels in a lane's run), F = 4 (one level) and F = 8 (half a level per lane, across a tile boundary): the same gate,
    both routes."""
    case, ref64, ref32 = to.references(("F", F))
    normals, grad = train_normals.analytic_normals(*_on(gpu, case), return_grad=True)
    _check(f"fused F={F} L={to.FEATURE_CASES[F][0]} {to.FEATURE_CASES[F][1]}", normals, grad, ref64, ref32)
    _check(f"composed F={F}", *train_normals.analytic_normals_composed(*_on(gpu, case), return_grad=True), ref64, ref32)


@pytest.mark.parametrize("L", [16, 5])
def test_fused_equals_composed_route(gpu, L):
    """The composed route under the same gate on the same inputs, and the two against each other."""
    case, ref64, ref32 = to.references(L)
    args = _on(gpu, case)
    cn, cg = train_normals.analytic_normals_composed(*args, return_grad=True)
    _check(f"composed L={L} {to.STACKS[L]}", cn, cg, ref64, ref32)
    fn, fg = train_normals.analytic_normals(*args, return_grad=True)
    det = to.determined(ref64)
    d_g, d_n = float((fg - cg).abs().max()), float((fn - cn)[det.to(gpu)].abs().max())
    print(f"fused - composed L={L}: grad_q max |d| {d_g:.2e}  normals max |d| {d_n:.2e}")
    # both routes hold the gate against ref64, so they lie within twice its limit of each other
    assert d_g <= 2 * to.gate(fg, ref64["g"], ref32["g"])[3] and d_n <= 2 * to.gate(fn, ref64["n"], ref32["n"], det)[3]


@pytest.mark.parametrize("L", [16, 5])
def test_normals_point_against_the_density_gradient(gpu, L):
    case, ref64, _ = to.references(L)
    normals = train_normals.analytic_normals(*_on(gpu, case)).cpu()
    want = -ref64["g"]
    # a component counts where it is well conditioned: above 1e-3 of the row's |g|, on the determined rows
    rows = to.determined(ref64)[:, None] & (want.abs() >= 1e-3 * want.norm(dim=-1, keepdim=True)) & (want != 0)
    assert int(rows.sum()) >= 0.9 * want.numel()
    assert torch.equal(torch.sign(normals)[rows].double(), torch.sign(want)[rows])


@pytest.mark.parametrize("L", [16, 5])
def test_a_zero_gradient_gives_a_zero_normal(gpu, L):
    """Row 0 of the last layer is zero: g_enc = 0, g = 0, and F.normalize's rule gives an exact 0, never 0 / 0."""
    for route in (train_normals.analytic_normals, train_normals.analytic_normals_composed):
        normals, grad = route(*_on(gpu, to.case(L, zero_row=True)), return_grad=True)
        assert bool((grad == 0).all()) and bool((normals == 0).all()) and not bool(torch.isnan(normals).any())


def _raw_call(gpu, args, N, normals, grad, dims=None, L=None):
    q, table, scalings, log2_T, weights, biases = args
    dims = dims or [weights[0].shape[1]] + [w.shape[0] for w in weights]
    desc = mlp._desc(dims, weights, biases)
    return _lib.load().sn_train_normals_analytic(q.data_ptr(), table.data_ptr(), scalings.data_ptr(), N, L or scalings.numel(), log2_T, table.shape[1],
                                                 C.byref(desc), normals, grad, torch.cuda.current_stream().cuda_stream)


def test_reproducible_and_non_finite_rows_stay_in_their_row(gpu):
    """Two calls give equal bits; a non-finite or out-of-domain q row gives a NaN row and leaves its neighbours and the guard bands
    around both outputs untouched."""
    case, ref64, _ = to.references(16)
    q, table, scalings, log2_T, weights, biases = _on(gpu, case)
    N = q.shape[0]
    a = train_normals.analytic_normals(q, table, scalings, log2_T, weights, biases, return_grad=True)
    b = train_normals.analytic_normals(q, table, scalings, log2_T, weights, biases, return_grad=True)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    bad = {7: float("nan"), 64: float("inf"), 65: -float("inf"), 500: 3.0e9, N - 1: float("nan")}
    qb = q.clone()
    for row, v in bad.items():
        qb[row, row % 3] = v
    bufs = [torch.full((3 * N + 2 * GUARD,), -777.0, device=gpu) for _ in range(2)]
    ptrs = [t.data_ptr() + 4 * GUARD for t in bufs]
    assert _raw_call(gpu, (qb, table, scalings, log2_T, weights, biases), N, *ptrs) == _lib.SN_OK
    torch.cuda.synchronize(gpu)
    keep = torch.ones(N, dtype=torch.bool, device=gpu)
    keep[list(bad)] = False
    for buf, want in zip(bufs, a):
        assert bool((buf[:GUARD] == -777.0).all()) and bool((buf[-GUARD:] == -777.0).all())
        got = buf[GUARD:-GUARD].view(N, 3)
        assert bool(torch.isnan(got[~keep]).all()) and torch.equal(got[keep].view(torch.int32), want[keep].view(torch.int32))


@pytest.mark.parametrize("N", [0, 1, 65])
def test_edge_sizes(gpu, N):
    """Nothing, one point, and one point more than a wave's 64 lanes (five 16-point tiles: two workgroups)."""
    case, ref64, ref32 = to.references(16)
    q, table, scalings, log2_T, weights, biases = _on(gpu, case)
    normals, grad = train_normals.analytic_normals(q[:N], table, scalings, log2_T, weights, biases, return_grad=True)
    assert normals.shape == grad.shape == (N, 3)
    if N == 0:
        assert _raw_call(gpu, (q, table, scalings, log2_T, weights, biases), 0, None, None) == _lib.SN_OK
        return
    full = train_normals.analytic_normals(q, table, scalings, log2_T, weights, biases, return_grad=True)
    assert torch.equal(normals.view(torch.int32), full[0][:N].view(torch.int32)) and torch.equal(grad.view(torch.int32), full[1][:N].view(torch.int32))
    assert to.gate(grad, ref64["g"][:N], ref32["g"][:N])[0]
    # leading dimensions are kept
    assert train_normals.analytic_normals(q[:N].reshape(1, N, 3), table, scalings, log2_T, weights, biases).shape == (1, N, 3)


def test_a_stack_that_does_not_fit_the_grid_is_refused_and_nothing_is_written(gpu):
    case, _, _ = to.references(16)
    args = _on(gpu, case)
    N = 65
    bufs = [torch.full((3 * N,), -777.0, device=gpu) for _ in range(2)]
    lib = _lib.load()
    # dims[0] = 32 beside L * F = 10 (L = 5), and a descriptor that says 10 beside L * F = 32
    assert _raw_call(gpu, args, N, bufs[0].data_ptr(), bufs[1].data_ptr(), L=5) == _lib.SN_ERR_INVALID
    assert b"sn_train_normals_analytic" in lib.sn_last_error(None) and b"L * F" in lib.sn_last_error(None)
    assert _raw_call(gpu, args, N, bufs[0].data_ptr(), bufs[1].data_ptr(), dims=[10, 64, 16]) == _lib.SN_ERR_INVALID
    assert _raw_call(gpu, args, 0, None, None, L=5) == _lib.SN_ERR_INVALID                 # (also at N = 0, like every range check)
    torch.cuda.synchronize(gpu)
    assert all(bool((t == -777.0).all()) for t in bufs)
    q, table, scalings, log2_T, weights, biases = args
    with pytest.raises(ValueError, match="weights\\[0\\]"):
        train_normals.analytic_normals(q, table[:5 << log2_T], scalings[:5], log2_T, weights, biases)
