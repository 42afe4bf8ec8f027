"""The trainable tiny-cuda-nn grid on the GPU (signerf_amd/hashgrid.py with grid="tcnn" over csrc/sn_hashgrid_tcnn.h) against
tests/tcnn_hashgrid_oracle.py.

Gates, the torch-path grid's own (tests/test_gpu_hashgrid.py; DESIGN.md §4 "Trainable hash grid"):
  idx         equal to the oracle's, bit for bit
  enc, grad_q e_hip <= 2 e_ref32 + 1 ulp of the largest output (e_hip, e_ref32: the kernel's and the fp32 restatement's largest error against
              the fp64 restatement)
  grad_table  per element |hip - ref64| <= (n + 4) 2^-24 A for n contributions with A = sum w |grad_enc|; exactly 0 where n = 0 -- which
              includes the unused tail of every dense level's slot

Every case runs with both forms of the table gradient's atomics, through the torch-path grid's switch: one add per corner ("plain") and
equal rows merged within the wave first ("merged": every level).  Each test prints its figures before it asserts."""
import os

import pytest
import torch

import hashgrid_oracle as ho
import tcnn_hashgrid_oracle as to
from oracle import tcnn_layout as tl
from signerf_amd import _lib, hashgrid
from signerf_amd.nerfacto import HashEncoding

pytestmark = pytest.mark.gpu

SMALL = (8, 13, 4, 64)      # 5 dense + 3 hashed levels; the dense index wraps past n_l on levels 0, 1, 2, 4
ONE = (1, 9, 8, 8)          # one dense level, r = 8
SHAPES = [(6, 12, 2, 40), ONE, (16, 10, 16, 2048), (5, 17, 16, 128), (16, 19, 16, 2048)]
# (name, (L, log2_T, base, max), F, N, kind of q, table scale)
CASES = [("L8_T13_N%d" % n, SMALL, 2, n, "uniform", 1.0) for n in (1, 63, 64, 65, 1000)]
CASES += [("L%d_T%d_N1000" % s[:2], s, 2, 1000, "uniform", 1.0) for s in SHAPES]
CASES += [("L8_T13_F%d" % f, SMALL, f, 1000, "uniform", 1.0) for f in (1, 4, 8)]
CASES += [("along_rays", SMALL, 2, 1000, "rays", 1.0), ("init_scale", SMALL, 2, 1000, "uniform", 1e-3),
          ("far_L8", SMALL, 2, 1000, "far", 1.0), ("far_L1", ONE, 2, 1000, "far", 1.0)]
FORMS = {"plain": "-1", "merged": "1e30"}
KW = dict(grid="tcnn")


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


def far_points(N, meta):
    """In-domain points far outside [0, 1]: x up to 2^29 at the finest level, so a dense level's index is many times n_l (a true modulo,
    not one subtraction) and, at r = 8, wraps uint32.  Row 0 of the one-level shape has x + 8 y + 64 z = 2^32 - 1 at corner 0: every other
    corner's 32-bit sum wraps."""
    q = torch.rand((N, 3), generator=torch.Generator().manual_seed(4)) * (2.0**29 / max(meta.scales))
    if meta.num_levels == 1 and meta.scales[0] == 7.0:
        q[0] = torch.tensor([1.0, 4.4, 9586980.0])         # floor(7 q + 0.5) = (7, 31, 2^26 - 4)
    return q


_REF = {}


def reference(name):
    """Inputs and CPU references of a case, computed once and shared by the tests that ask for it (the full-size table is not kept)."""
    if name not in _REF:
        _REF.pop("L16_T19_N1000", None)
        _, (L, log2_T, base, mx), F, N, kind, scale = next(c for c in CASES if c[0] == name)
        meta = tl.grid_meta(L, base, mx, log2_T, F)
        q = {"uniform": lambda: to.points(N, seed=N + L, meta=meta), "rays": lambda: to.ray_points(N, 5), "far": lambda: far_points(N, meta)}[kind]()
        assert bool(to.in_domain(q, meta).all())
        table, s = to.table(meta, F, seed=11, scale=scale), to.scalings(meta)
        g = torch.randn(N, L * F, generator=torch.Generator().manual_seed(2))
        enc64, idx = to.encode(q, table, meta, torch.float64)
        enc32, _ = to.encode(q, table, meta, torch.float32)
        gt64, gq64 = to.grads(q, table, meta, g, torch.float64)
        gt32, gq32 = to.grads(q, table, meta, g, torch.float32)
        n, A = to.contributions(idx, to.cells(q, meta)[1], g, table.shape[0])
        assert bool((n[~to.used_rows(meta)] == 0).all())
        _REF[name] = dict(q=q, table=table, s=s, g=g, log2_T=log2_T, meta=meta, idx=idx, enc64=enc64, enc32=enc32, gt64=gt64, gt32=gt32, gq64=gq64,
                          gq32=gq32, n=n, A=A)
    return _REF[name]


def table_error(got, r, calls=1):
    """-> (largest error / bound over the elements with contributions, the n = 0 elements are exactly 0)."""
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
    enc, idx = hashgrid.hash_corner_indices(q, table, s, r["log2_T"], **KW)
    gt, gq = hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, torch.zeros_like(table), want_grad_q=True, **KW)
    idx_equal = torch.equal(idx.cpu().to(torch.int64), r["idx"])
    ok_enc, e_enc, e_enc32, lim_enc = ho.gate(enc.cpu(), r["enc64"], r["enc32"])
    ok_gq, e_gq, e_gq32, lim_gq = ho.gate(gq.cpu(), r["gq64"], r["gq32"])
    ratio, zeros = table_error(gt, r)
    ref32_ratio, _ = table_error(r["gt32"], r)
    tail_zero = bool((gt.cpu()[~to.used_rows(r["meta"])] == 0).all())
    print(f"\n[tcnn hashgrid {name} {form}] idx equal {idx_equal} | enc e_hip {e_enc:.3e} e_ref32 {e_enc32:.3e} limit {lim_enc:.3e} | grad_q e_hip "
          f"{e_gq:.3e} e_ref32 {e_gq32:.3e} limit {lim_gq:.3e} | grad_table error/bound hip {ratio:.3f} ref32 {ref32_ratio:.3f}, untouched rows zero "
          f"{zeros}, tails of dense slots zero {tail_zero}")
    assert idx_equal
    assert ok_enc, (e_enc, e_enc32, lim_enc)
    assert ok_gq, (e_gq, e_gq32, lim_gq)
    assert ratio <= 1.0 and zeros and tail_zero, (ratio, zeros, tail_zero)
    # the autograd Function returns what the entry points returned
    qa, ta = q.clone().requires_grad_(), table.clone().requires_grad_()
    out = hashgrid.hash_encode(qa, ta, s, r["log2_T"], **KW)
    assert torch.equal(out, enc)
    out.backward(g)
    assert torch.equal(qa.grad, gq) and table_error(ta.grad, r)[0] <= 1.0


@pytest.mark.parametrize("name", ["L8_T13_N1000", "L16_T10_N1000"])
def test_backward_accumulates_and_takes_either_output_alone(gpu, form, name):
    r = reference(name)
    q, table, s, g = (r[k].to(gpu) for k in ("q", "table", "s", "g"))
    both_t, both_q = hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, torch.zeros_like(table), want_grad_q=True, **KW)
    only_t, none_q = hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, torch.zeros_like(table), want_grad_q=False, **KW)
    none_t, only_q = hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, None, want_grad_q=True, **KW)
    assert none_q is None and none_t is None and torch.equal(only_q, both_q)
    one = table_error(only_t, r)[0]
    buf = torch.zeros_like(table)
    for _ in range(2):
        hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, buf, **KW)
    two, zeros = table_error(buf, r, calls=2)
    print(f"\n[tcnn hashgrid accumulate {name} {form}] error/bound one call {one:.3f}, two calls into one buffer {two:.3f}")
    assert one <= 1.0 and two <= 1.0 and zeros


def test_out_of_domain_points_touch_nothing_else(gpu, form):
    r = reference("L8_T13_N1000")
    nan, inf = float("nan"), float("inf")
    top = max(r["meta"].scales)
    bad = torch.tensor([[nan, 0.5, 0.5], [0.5, inf, 0.5], [0.5, 0.5, -inf], [1e30, 0.5, 0.5], [0.5, -0.25, 0.5], [nan, inf, 1e30],
                        [0.5, 0.5, 1.01 * 2.0**30 / top], [-0.25, 0.1, 0.2]])
    assert not bool(to.in_domain(bad, r["meta"]).any())
    at = torch.tensor([0, 1, 64, 65, 500, 997, 998, 999])              # where the bad rows go in the longer batch
    N = r["q"].shape[0] + len(bad)
    clean = torch.ones(N, dtype=torch.bool)
    clean[at + torch.arange(len(at))] = False
    q_all, g_all = torch.empty(N, 3), torch.randn(N, r["g"].shape[1], generator=torch.Generator().manual_seed(9))
    q_all[clean], q_all[~clean] = r["q"], bad
    g_all[clean] = r["g"]
    table, s = r["table"].to(gpu), r["s"].to(gpu)
    enc0, idx0 = hashgrid.hash_corner_indices(r["q"].to(gpu), table, s, r["log2_T"], **KW)
    _, gq0 = hashgrid.hash_encode_backward(r["q"].to(gpu), table, s, r["log2_T"], r["g"].to(gpu), None, want_grad_q=True, **KW)
    enc, idx = hashgrid.hash_corner_indices(q_all.to(gpu), table, s, r["log2_T"], **KW)
    gt, gq = hashgrid.hash_encode_backward(q_all.to(gpu), table, s, r["log2_T"], g_all.to(gpu), torch.zeros_like(table), want_grad_q=True, **KW)
    clean_d = clean.to(gpu)
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    assert torch.equal(bits(enc[clean_d]), bits(enc0)) and torch.equal(idx[clean_d], idx0) and torch.equal(bits(gq[clean_d]), bits(gq0))
    assert bool(torch.isnan(enc[~clean_d]).all()) and bool((idx[~clean_d] == 0).all()) and bool(torch.isnan(gq[~clean_d]).all())
    ratio, zeros = table_error(gt, r)
    print(f"\n[tcnn hashgrid out of domain {form}] grad_table error/bound against the clean batch {ratio:.3f}")
    assert bool(torch.isfinite(gt).all()) and ratio <= 1.0 and zeros


def test_features_and_input_gradient_are_reproducible(gpu, form):
    r = reference("L8_T13_N1000")
    q, table, s, g = (r[k].to(gpu) for k in ("q", "table", "s", "g"))
    runs = [(hashgrid.hash_corner_indices(q, table, s, r["log2_T"], **KW),
             hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, None, True, **KW)[1]) for _ in range(2)]
    (e0, i0), q0 = runs[0]
    (e1, i1), q1 = runs[1]
    assert torch.equal(e0.view(torch.int32), e1.view(torch.int32)) and torch.equal(i0, i1) and torch.equal(q0.view(torch.int32), q1.view(torch.int32))


def test_autograd_wiring(gpu):
    torch.manual_seed(0)
    enc = HashEncoding(5, 16, 128, 12, implementation="tcnn").to(gpu)
    q = torch.rand(6, 7, 3, device=gpu)
    with pytest.raises(NotImplementedError, match="tiny-cuda-nn"):     # off until the owning model switches it on
        enc(q)
    enc.trainable_tcnn = True
    out = enc(q)
    assert out.shape == (6, 7, 10) and out.requires_grad
    out.sum().backward()
    meta = tl.grid_meta(5, 16, 128, 12)
    grad = enc.hash_table.grad
    assert grad.shape == enc.hash_table.shape and float(grad.abs().sum()) > 0 and bool((grad.cpu()[~to.used_rows(meta)] == 0).all())
    assert list(enc.state_dict()) == ["hash_table"]
    # leading dimensions: the same rows as the flat batch
    assert torch.equal(enc(q.reshape(-1, 3)).reshape(6, 7, 10), out)
    # the oracle's value on the library's own layout, through the module
    want = tl.grid_encode(q.reshape(-1, 3).cpu(), to.flat_rows(enc.hash_table.detach().cpu(), meta), meta)
    assert torch.equal(out.detach().reshape(-1, 10).cpu(), want)
    # the function, with and without a gradient in q
    assert torch.equal(hashgrid.hash_encode(q, enc.hash_table, enc._scalings_on(q.device), 12, grid="tcnn"), out)
    qg = q.clone().requires_grad_()
    enc(qg).sum().backward()
    assert qg.grad.shape == q.shape and bool(torch.isfinite(qg.grad).all()) and float(qg.grad.abs().max()) > 0
    # N = 0
    empty = enc(torch.empty(0, 3, device=gpu))
    assert empty.shape == (0, 10)
    enc.hash_table.grad = None
    empty.sum().backward()
    assert float(enc.hash_table.grad.abs().sum()) == 0.0
    # second order is refused, not silently wrong
    w = torch.ones(6, 7, 10, device=gpu, requires_grad=True)
    g2, = torch.autograd.grad((enc(qg) * w).sum(), qg, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g2.sum().backward()
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        enc(q.cpu())
