"""The trainable hash grid on the GPU (signerf_amd/hashgrid.py over csrc/sn_hashgrid.h) against tests/hashgrid_oracle.py.

Gates (DESIGN.md §4 "Trainable hash grid"):
  idx         equal to the oracle's, bit for bit
  enc, grad_q e_hip <= 2 e_ref32 + 1 ulp of the largest output (e_hip, e_ref32: the kernel's and the fp32 restatement's largest error against
              the fp64 restatement)
  grad_table  per element |hip - ref64| <= (n + 4) 2^-24 A for n contributions with A = sum w |grad_enc|; exactly 0 where n = 0

Every case runs with both forms of the table gradient's atomics: one add per corner ("plain") and equal rows merged within the wave first
("merged": every level, whatever threshold the library ships with).  Each test prints its figures before it asserts."""
import os

import pytest
import torch

import hashgrid_oracle as ho
from helpers import onf
from signerf_amd import _lib, hashgrid
from signerf_amd.nerfacto import HashEncoding, MLPWithHashEncoding

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 16, 16), (5, 1, 16, 128), (16, 4, 16, 2048), (16, 10, 16, 2048), (5, 17, 16, 128)]
# (name, (L, log2_T, base, max), F, N, (lo, hi) of q, table scale)
CASES = [("L%d_T%d_N%d" % (s[0], s[1], n), s, 2, n, (0.0, 1.0), 1.0) for s in SHAPES for n in (1, 63, 64, 65, 1000)]
CASES += [("L16_T4_F%d" % f, SHAPES[2], f, 1000, (0.0, 1.0), 1.0) for f in (1, 4, 8)]
CASES += [("main_table", (16, 19, 16, 2048), 2, 1000, (0.0, 1.0), 1.0),
          ("negative_coordinates", SHAPES[3], 2, 1000, (-0.5, 1.5), 1.0),
          ("init_scale", SHAPES[3], 2, 1000, (0.0, 1.0), 1e-3),
          ("along_rays", SHAPES[3], 2, 1000, None, 1.0)]
FORMS = {"plain": "-1", "merged": "1e30"}


@pytest.fixture(params=list(FORMS))
def form(request, gpu):
    """Selects the form of the table gradient's atomics for the test (include/signerf_hip_hashgrid.h, sn_hashgrid_debug_reload_env)."""
    lib = _lib.load()
    old = os.environ.get("SN_HASHGRID_MERGE_MAX_SCALE")
    os.environ["SN_HASHGRID_MERGE_MAX_SCALE"] = FORMS[request.param]
    assert lib.sn_hashgrid_debug_reload_env() == 0
    yield request.param
    if old is None:
        del os.environ["SN_HASHGRID_MERGE_MAX_SCALE"]
    else:
        os.environ["SN_HASHGRID_MERGE_MAX_SCALE"] = old
    assert lib.sn_hashgrid_debug_reload_env() == 0


def ray_points(N, seed):
    """Consecutive samples of a few rays through the unit cube, 200 per ray: neighbours share cells on the coarse levels."""
    g = torch.Generator().manual_seed(seed)
    rays = (N + 199) // 200
    a, b = torch.rand(rays, 1, 3, generator=g), torch.rand(rays, 1, 3, generator=g)
    t = torch.linspace(0.0, 1.0, 200).view(1, 200, 1)
    return (a + (b - a) * t).reshape(-1, 3)[:N].contiguous()


_REF = {}


def reference(name):
    """Inputs and CPU references of a case, computed once and shared by the tests that ask for it (the full-size table is not kept)."""
    if name not in _REF:
        _REF.pop("main_table", None)
        _, (L, log2_T, base, mx), F, N, rng, scale = next(c for c in CASES if c[0] == name)
        q = ray_points(N, 5) if rng is None else ho.points(N, seed=N + L, lo=rng[0], hi=rng[1])
        table, s = ho.table(L, log2_T, F, seed=11, scale=scale), onf.hash_scalings(L, base, mx)
        g = torch.randn(N, L * F, generator=torch.Generator().manual_seed(2))
        enc64, idx = ho.encode(q, table, s, log2_T, torch.float64)
        enc32, _ = ho.encode(q, table, s, log2_T, torch.float32)
        gt64, gq64 = ho.grads(q, table, s, log2_T, g, torch.float64)
        gt32, gq32 = ho.grads(q, table, s, log2_T, g, torch.float32)
        n, A = ho.contributions(idx, ho.cells(q, s, log2_T)[1], g, table.shape[0])
        _REF[name] = dict(q=q, table=table, s=s, g=g, log2_T=log2_T, idx=idx, enc64=enc64, enc32=enc32, gt64=gt64, gt32=gt32, gq64=gq64, gq32=gq32,
                          n=n, A=A)
    return _REF[name]


def table_error(got, r, calls=1):
    """-> (largest error / bound over the elements with contributions, the n = 0 elements are exactly 0).  `calls` backward passes into one
    buffer are calls * n contributions with calls * A: the same bound, for the doubled list."""
    n, A = r["n"] * calls, r["A"] * calls
    err = (got.double().cpu() - calls * r["gt64"]).abs()
    bound = ho.grad_table_bound(n, A)
    hit = n > 0
    ratio = float((err[hit] / bound[hit].clamp_min(1e-300)).max()) if bool(hit.any()) else 0.0
    if bool((A[hit] == 0).any()):     # a contribution list of zero weights: the bound is 0 and so must the error be
        ratio = max(ratio, float("inf") if bool((err[hit][A[hit] == 0] != 0).any()) else 0.0)
    return ratio, bool((got.cpu()[~hit] == 0).all())


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_forward_and_backward_against_the_restatement(gpu, form, name):
    r = reference(name)
    q, table, s, g = (r[k].to(gpu) for k in ("q", "table", "s", "g"))
    enc, idx = hashgrid.hash_corner_indices(q, table, s, r["log2_T"])
    gt, gq = hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, torch.zeros_like(table), want_grad_q=True)
    idx_equal = torch.equal(idx.cpu().to(torch.int64), r["idx"])
    ok_enc, e_enc, e_enc32, lim_enc = ho.gate(enc.cpu(), r["enc64"], r["enc32"])
    ok_gq, e_gq, e_gq32, lim_gq = ho.gate(gq.cpu(), r["gq64"], r["gq32"])
    ratio, zeros = table_error(gt, r)
    ref32_ratio, _ = table_error(r["gt32"], r)
    print(f"\n[hashgrid {name} {form}] idx equal {idx_equal} | enc e_hip {e_enc:.3e} e_ref32 {e_enc32:.3e} limit {lim_enc:.3e} | grad_q e_hip {e_gq:.3e} "
          f"e_ref32 {e_gq32:.3e} limit {lim_gq:.3e} | grad_table error/bound hip {ratio:.3f} ref32 {ref32_ratio:.3f}, untouched rows zero {zeros}")
    assert idx_equal
    assert ok_enc, (e_enc, e_enc32, lim_enc)
    assert ok_gq, (e_gq, e_gq32, lim_gq)
    assert ratio <= 1.0 and zeros, (ratio, zeros)
    # the autograd Function returns what the entry points returned
    qa, ta = q.clone().requires_grad_(), table.clone().requires_grad_()
    out = hashgrid.hash_encode(qa, ta, s, r["log2_T"])
    assert torch.equal(out, enc)
    out.backward(g)
    assert torch.equal(qa.grad, gq) and table_error(ta.grad, r)[0] <= 1.0


@pytest.mark.parametrize("name", ["L5_T1_N1000", "L16_T10_N1000"])
def test_backward_accumulates_and_takes_either_output_alone(gpu, form, name):
    r = reference(name)
    q, table, s, g = (r[k].to(gpu) for k in ("q", "table", "s", "g"))
    both_t, both_q = hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, torch.zeros_like(table), want_grad_q=True)
    only_t, none_q = hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, torch.zeros_like(table), want_grad_q=False)
    none_t, only_q = hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, None, want_grad_q=True)
    assert none_q is None and none_t is None and torch.equal(only_q, both_q)
    one = table_error(only_t, r)[0]
    buf = torch.zeros_like(table)
    for _ in range(2):
        hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, buf)
    two, zeros = table_error(buf, r, calls=2)
    print(f"\n[hashgrid accumulate {name} {form}] error/bound one call {one:.3f}, two calls into one buffer {two:.3f}")
    assert one <= 1.0 and two <= 1.0 and zeros


def test_out_of_domain_points_touch_nothing_else(gpu, form):
    r = reference("L16_T10_N1000")
    nan, inf = float("nan"), float("inf")
    bad = torch.tensor([[nan, 0.5, 0.5], [0.5, inf, 0.5], [0.5, 0.5, -inf], [1e30, 0.5, 0.5], [0.5, -1e30, 0.5], [nan, inf, 1e30],
                        [0.5, 0.5, 2.0**30 / 16], [-2.0**30 / 16, 0.1, 0.2]])
    at = torch.tensor([0, 1, 64, 65, 500, 997, 998, 999])              # where the bad rows go in the longer batch
    N = r["q"].shape[0] + len(bad)
    clean = torch.ones(N, dtype=torch.bool)
    clean[at + torch.arange(len(at))] = False
    q_all, g_all = torch.empty(N, 3), torch.randn(N, r["g"].shape[1], generator=torch.Generator().manual_seed(9))
    q_all[clean], q_all[~clean] = r["q"], bad
    g_all[clean] = r["g"]
    table, s = r["table"].to(gpu), r["s"].to(gpu)
    enc0, idx0 = hashgrid.hash_corner_indices(r["q"].to(gpu), table, s, r["log2_T"])
    _, gq0 = hashgrid.hash_encode_backward(r["q"].to(gpu), table, s, r["log2_T"], r["g"].to(gpu), None, want_grad_q=True)
    enc, idx = hashgrid.hash_corner_indices(q_all.to(gpu), table, s, r["log2_T"])
    gt, gq = hashgrid.hash_encode_backward(q_all.to(gpu), table, s, r["log2_T"], g_all.to(gpu), torch.zeros_like(table), want_grad_q=True)
    clean_d = clean.to(gpu)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    assert torch.equal(bits(enc[clean_d]), bits(enc0)) and torch.equal(idx[clean_d], idx0) and torch.equal(bits(gq[clean_d]), bits(gq0))
    assert bool(torch.isnan(enc[~clean_d]).all()) and bool((idx[~clean_d] == 0).all()) and bool(torch.isnan(gq[~clean_d]).all())
    ratio, zeros = table_error(gt, r)
    print(f"\n[hashgrid out of domain {form}] grad_table error/bound against the clean batch {ratio:.3f}")
    assert bool(torch.isfinite(gt).all()) and ratio <= 1.0 and zeros


def test_features_and_input_gradient_are_reproducible(gpu, form):
    r = reference("L16_T10_N1000")
    q, table, s, g = (r[k].to(gpu) for k in ("q", "table", "s", "g"))
    runs = [(hashgrid.hash_corner_indices(q, table, s, r["log2_T"]), hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, None, True)[1])
            for _ in range(2)]
    (e0, i0), q0 = runs[0]
    (e1, i1), q1 = runs[1]
    assert torch.equal(e0.view(torch.int32), e1.view(torch.int32)) and torch.equal(i0, i1) and torch.equal(q0.view(torch.int32), q1.view(torch.int32))


def test_autograd_wiring(gpu):
    torch.manual_seed(0)
    enc = HashEncoding(5, 16, 128, 10).to(gpu)
    q = torch.rand(6, 7, 3, device=gpu)
    out = enc(q)
    assert out.shape == (6, 7, 10) and out.requires_grad
    out.sum().backward()
    assert enc.hash_table.grad.shape == enc.hash_table.shape and float(enc.hash_table.grad.abs().sum()) > 0
    assert list(enc.state_dict()) == ["hash_table"]
    # leading dimensions: the same rows as the flat batch
    assert torch.equal(enc(q.reshape(-1, 3)).reshape(6, 7, 10), out)
    # the oracle's value, through the module
    want = onf.hash_encode(q.reshape(-1, 3).cpu(), enc.hash_table.detach().cpu(), enc.scalings(), 10)
    assert torch.equal(out.detach().reshape(-1, 10).cpu(), want)
    # q gets a gradient only when it asks for one
    qg = q.clone().requires_grad_()
    enc(qg).sum().backward()
    assert qg.grad.shape == q.shape and bool(torch.isfinite(qg.grad).all())
    # N = 0
    empty = enc(torch.empty(0, 3, device=gpu))
    assert empty.shape == (0, 10)
    enc.hash_table.grad = None
    empty.sum().backward()
    assert float(enc.hash_table.grad.abs().sum()) == 0.0
    # second order is refused, not silently wrong: the first-order gradient of a once_differentiable Function carries no graph when its
    # incoming gradient has none, and a node that raises when it has one
    g1, = torch.autograd.grad(enc(qg).sum(), qg, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        g1.sum().backward()
    w = torch.ones(6, 7, 10, device=gpu, requires_grad=True)
    g2, = torch.autograd.grad((enc(qg) * w).sum(), qg, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g2.sum().backward()
    # a CPU module on a GPU tensor is torch's business; a GPU module on a CPU tensor is refused by the op
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        enc(q.cpu())


def test_a_small_field_fits_a_function(gpu):
    """MLPWithHashEncoding + Adam, 40 steps on 4096 fixed points: the final MSE is at most half the initial one (the oracle's own encoding,
    fitted the same way on the CPU, ends at 0.21 to 0.27 of it)."""
    torch.manual_seed(0)
    net = MLPWithHashEncoding(4, 16, 128, 10, 2, 2, 16, 1).to(gpu)
    q = torch.rand(4096, 3, generator=torch.Generator().manual_seed(1)).to(gpu)
    target = (torch.sin(6 * q[:, 0]) * torch.cos(5 * q[:, 1]) + q[:, 2])[:, None]
    opt = torch.optim.Adam(net.parameters(), lr=1e-2, eps=1e-15)
    history = []
    for _ in range(40):
        opt.zero_grad()
        loss = torch.mean((net(q) - target) ** 2)
        loss.backward()
        opt.step()
        history.append(loss.detach())
    with torch.no_grad():
        final = float(torch.mean((net(q) - target) ** 2))
    first = float(history[0])
    print(f"\n[hashgrid fit] mse {first:.4f} -> {final:.4f} ({final / first:.3f} of the initial)")
    assert final <= 0.5 * first
