"""The ordered table gradient of both trainable hash grids on the GPU (hashgrid.hash_encode*(table_grad="ordered") over
csrc/sn_hashgrid_ordered.h; signerf_amd/include/signerf_hip_hashgrid_ordered.h) against the fp64 autograd of tests/hashgrid_oracle.py and
tests/tcnn_hashgrid_oracle.py.

Gates (DESIGN.md §4 "Ordered table gradient"):
  grad_table  per element with n contributions and A = sum w |grad_enc|: |hip - ref64| <= (2 + n 2^-29) 2^-24 A -- one fp32 rounding of
              every product, an fp64 sum, one final fp32 rounding; independent of n for any batch that fits.  An element without a
              contribution holds exactly what the buffer held.
              Into a buffer that holds a value s already, the final rounding is that of s + S: (1 + n 2^-29) 2^-24 A + 2^-24 (|s| + A).
              For `calls` calls into one zeroed buffer, with n and A counting everything added to it (as tests/test_gpu_hashgrid.py counts):
              (2 calls + n 2^-29) 2^-24 A; call k rounds its products (1 / calls of A) and a running sum of at most k / calls of A, so
              the roundings add up to (1 + (calls + 1) / 2) 2^-24 A, which is <= 2 calls 2^-24 A.
  bits        repeated calls, calls on another stream, calls with SN_HASHGRID_MERGE_MAX_SCALE changed: identical.  grad_q: identical to the
              atomic entry point's.
Every test prints its figures before it asserts."""
import os
import sys

import pytest
import torch

import hashgrid_oracle as ho
import tcnn_hashgrid_oracle as to
from helpers import ROOT, small_config
from oracle import nerfacto as onf
from oracle import tcnn_layout as tl
from signerf_amd import _lib, hashgrid
from signerf_amd.nerfacto import HashEncoding

pytestmark = pytest.mark.gpu

GRIDS = ("torch", "tcnn")
NS = (1, 63, 65, 257, 5000)
# name -> (L, log2_T, base_res, max_res): every row collides and the segments are longer than a workgroup; nerfacto's main grid; one level
# over the largest table, so that every radix pass runs (scale 1024: hashed in both grids, the keys spread over all 24 bits)
LEVELS = {"collide": (5, 4, 16, 128), "nerfacto": (16, 19, 16, 2048), "wide": (1, 24, 1024, 1024)}
CASES = [("collide", F, N) for F in (1, 2, 4, 8) for N in NS] + [("nerfacto", 2, N) for N in NS] + [("wide", 1, N) for N in NS]
SENTINEL = -3.25
bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731


def ordered_bound(n, A, calls=1):
    return (2.0 * calls + n.double() * 2.0**-29) * 2.0**-24 * A


_REF = {}


def reference(grid, levels, F, N, g_kind="randn"):
    """Inputs and the CPU references of a case, computed once and shared; of the cases on a large table only the last is kept."""
    key = (grid, levels, F, N, g_kind)
    if key not in _REF:
        for k in [k for k in _REF if k[1] != "collide"]:
            del _REF[k]
        L, log2_T, base, mx = LEVELS[levels]
        gen = torch.Generator().manual_seed(1000 * N + 10 * F + L)
        if g_kind == "randn":
            g = torch.randn(N, L * F, generator=gen)
        elif g_kind == "positive":
            g = torch.rand(N, L * F, generator=gen) + 0.5
        else:   # magnitudes over 2^-20 .. 2^20, mixed signs
            g = torch.randn(N, L * F, generator=gen) * torch.exp2(torch.rand(N, L * F, generator=gen) * 40 - 20)
        if grid == "torch":
            q, s = ho.points(N, seed=N + L), onf.hash_scalings(L, base, mx)
            table = ho.table(L, log2_T, F, seed=11)
            idx, offset = ho.cells(q, s, log2_T)
            gt64, _ = ho.grads(q, table, s, log2_T, g, torch.float64)
            n, A = ho.contributions(idx, offset, g, table.shape[0])
        else:
            meta = tl.grid_meta(L, base, mx, log2_T, F)
            q, s = to.points(N, seed=N + L, meta=meta), to.scalings(meta)
            table = to.table(meta, F, seed=11)
            idx, w, _ = to.cells(q, meta)
            gt64, _ = to.grads(q, table, meta, g, torch.float64)
            n, A = to.contributions(idx, w, g, table.shape[0])
        _REF[key] = dict(q=q, table=table, s=s, g=g, log2_T=log2_T, gt64=gt64, n=n, A=A)
    return _REF[key]


def table_error(got, r, calls=1, prior=0.0):
    """-> (the largest error / bound over the elements with contributions, the elements without one hold `prior` exactly)."""
    n, A = r["n"] * calls, r["A"] * calls
    got = got.cpu()
    err = (got.double() - (calls * r["gt64"] + prior)).abs()
    bound = ordered_bound(n, A, calls) if prior == 0.0 else (1.0 + n.double() * 2.0**-29) * 2.0**-24 * A + 2.0**-24 * (abs(prior) + A)
    hit = n > 0
    ratio = float((err[hit] / bound[hit].clamp_min(1e-300)).max())
    if bool((bound[hit] == 0).any()):     # a contribution list of zero weights: the bound is 0 and so must the error be
        ratio = max(ratio, float("inf") if bool((err[hit][bound[hit] == 0] != 0).any()) else 0.0)
    untouched = torch.equal(bits(got[~hit]), bits(torch.full_like(got[~hit], prior)))
    return ratio, untouched


def backward(r, gpu, grid, buf=None, want_grad_q=False, table_grad="ordered", g=None):
    q, table, s = (r[k].to(gpu) for k in ("q", "table", "s"))
    g = (r["g"] if g is None else g).to(gpu)
    buf = torch.zeros_like(table) if buf is None else buf
    return hashgrid.hash_encode_backward(q, table, s, r["log2_T"], g, buf, want_grad_q=want_grad_q, grid=grid, table_grad=table_grad)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("levels,F,N", CASES)
def test_parity_and_the_tight_bound(gpu, grid, levels, F, N):
    r = reference(grid, levels, F, N)
    gt, gq = backward(r, gpu, grid, want_grad_q=True)
    ratio, untouched = table_error(gt, r)
    filled, _ = backward(r, gpu, grid, buf=torch.full_like(r["table"], SENTINEL).to(gpu))
    s_ratio, s_untouched = table_error(filled, r, prior=SENTINEL)
    _, gq_atomic = hashgrid.hash_encode_backward(r["q"].to(gpu), r["table"].to(gpu), r["s"].to(gpu), r["log2_T"], r["g"].to(gpu), None, want_grad_q=True,
                                                 grid=grid)
    same_q = torch.equal(bits(gq), bits(gq_atomic))
    print(f"\n[ordered {grid} {levels} F{F} N{N}] contributions per element up to {int(r['n'].max())}; error / bound {ratio:.3f}, untouched rows "
          f"untouched {untouched}; into a buffer of {SENTINEL}: {s_ratio:.3f}, {s_untouched}; grad_q equals the atomic entry point's {same_q}")
    assert ratio <= 1.0 and untouched, (ratio, untouched)
    assert s_ratio <= 1.0 and s_untouched, (s_ratio, s_untouched)
    assert same_q


@pytest.mark.parametrize("grid", GRIDS)
def test_two_calls_give_the_same_bits(gpu, grid):
    lib = _lib.load()
    for g_kind in ("positive", "spread"):
        r = reference(grid, "collide", 2, 5000, g_kind)
        runs = [backward(r, gpu, grid)[0] for _ in range(5)]
        ratio, untouched = table_error(runs[0], r)
        side = torch.cuda.Stream(device=gpu)
        side.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.stream(side):
            runs.append(backward(r, gpu, grid)[0])
        side.synchronize()
        old = os.environ.get("SN_HASHGRID_MERGE_MAX_SCALE")
        os.environ["SN_HASHGRID_MERGE_MAX_SCALE"] = "-1"
        try:
            assert lib.sn_hashgrid_debug_reload_env() == 0
            runs.append(backward(r, gpu, grid)[0])
            atomic_plain = backward(r, gpu, grid, table_grad="atomic")[0]
        finally:
            if old is None:
                del os.environ["SN_HASHGRID_MERGE_MAX_SCALE"]
            else:
                os.environ["SN_HASHGRID_MERGE_MAX_SCALE"] = old
            assert lib.sn_hashgrid_debug_reload_env() == 0
        atomic = [backward(r, gpu, grid, table_grad="atomic")[0] for _ in range(2)]
        differs = [int((bits(a) != bits(runs[0])).sum()) for a in (atomic[0], atomic[1], atomic_plain)]
        print(f"\n[ordered reproducible {grid} {g_kind}] 5 calls, a side stream, another merge threshold: identical "
              f"{[torch.equal(bits(x), bits(runs[0])) for x in runs[1:]]}; error / bound {ratio:.3f}; elements (of {runs[0].numel()}) on which the "
              f"atomic form differs from it: shipped {differs[0]} and {differs[1]}, plain {differs[2]}; two atomic calls differ from each other on "
              f"{int((bits(atomic[0]) != bits(atomic[1])).sum())}")
        assert ratio <= 1.0 and untouched
        assert all(torch.equal(bits(x), bits(runs[0])) for x in runs[1:])


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("levels,F,N", [("collide", 2, 5000), ("nerfacto", 2, 257)])
def test_backward_accumulates_and_takes_either_output_alone(gpu, grid, levels, F, N):
    r = reference(grid, levels, F, N)
    both_t, both_q = backward(r, gpu, grid, want_grad_q=True)
    only_t, none_q = backward(r, gpu, grid)
    none_t, only_q = hashgrid.hash_encode_backward(r["q"].to(gpu), r["table"].to(gpu), r["s"].to(gpu), r["log2_T"], r["g"].to(gpu), None, want_grad_q=True,
                                                   grid=grid, table_grad="ordered")
    assert none_q is None and none_t is None
    assert torch.equal(bits(only_q), bits(both_q)) and torch.equal(bits(only_t), bits(both_t))
    twice = []
    for _ in range(2):
        buf = torch.zeros_like(r["table"]).to(gpu)
        for _ in range(2):
            backward(r, gpu, grid, buf=buf)
        twice.append(buf)
    two, untouched = table_error(twice[0], r, calls=2)
    print(f"\n[ordered accumulate {grid} {levels}] two calls into one buffer: error / bound {two:.3f}; the same bits again "
          f"{torch.equal(bits(twice[0]), bits(twice[1]))}")
    assert two <= 1.0 and untouched and torch.equal(bits(twice[0]), bits(twice[1]))


@pytest.mark.parametrize("grid", GRIDS)
def test_out_of_domain_points_change_no_bit(gpu, grid):
    """NaN, +-inf and 2^31 rows between the clean ones: grad_table is bit for bit the clean batch's (the lists keep their order; the atomic
    form could only bound this)."""
    r = reference(grid, "collide", 2, 5000)
    nan, inf = float("nan"), float("inf")
    bad = torch.tensor([[nan, 0.5, 0.5], [0.5, inf, 0.5], [0.5, 0.5, -inf], [2.0**31, 0.5, 0.5], [0.5, -(2.0**31), 0.5], [nan, inf, 2.0**31],
                        [0.5, 0.5, 2.0**31], [-(2.0**31), 0.1, 0.2]])
    at = torch.tensor([0, 1, 64, 65, 2500, 4997, 4998, 4999])
    N = r["q"].shape[0] + len(bad)
    clean = torch.ones(N, dtype=torch.bool)
    clean[at + torch.arange(len(at))] = False
    q_all, g_all = torch.empty(N, 3), torch.randn(N, r["g"].shape[1], generator=torch.Generator().manual_seed(9))
    q_all[clean], q_all[~clean] = r["q"], bad
    g_all[clean] = r["g"]
    want, _ = backward(r, gpu, grid)
    table, s = r["table"].to(gpu), r["s"].to(gpu)
    got, gq = hashgrid.hash_encode_backward(q_all.to(gpu), table, s, r["log2_T"], g_all.to(gpu), torch.zeros_like(table), want_grad_q=True, grid=grid,
                                            table_grad="ordered")
    same = torch.equal(bits(got), bits(want))
    print(f"\n[ordered out of domain {grid}] grad_table equals the clean batch's bit for bit: {same}")
    assert same and bool(torch.isnan(gq[~clean.to(gpu)]).all()) and bool(torch.isfinite(gq[clean.to(gpu)]).all())


@pytest.mark.parametrize("grid", GRIDS)
def test_autograd_wiring(gpu, grid):
    torch.manual_seed(0)
    enc = HashEncoding(5, 16, 128, 10, implementation=grid).to(gpu)
    enc.trainable_tcnn = grid == "tcnn"
    q = torch.rand(6, 7, 3, device=gpu)
    atomic = enc(q)
    enc.table_grad = "ordered"
    out = enc(q)
    assert out.requires_grad and torch.equal(bits(out.detach()), bits(atomic.detach()))
    g = torch.randn_like(out)
    grads = []
    for _ in range(2):
        enc.hash_table.grad = None
        enc(q).backward(g)
        grads.append(enc.hash_table.grad.clone())
    assert torch.equal(bits(grads[0]), bits(grads[1])) and float(grads[0].abs().sum()) > 0
    enc.table_grad = "atomic"
    enc.hash_table.grad = None
    enc(q).backward(g)
    close = float((enc.hash_table.grad - grads[0]).abs().max())
    print(f"\n[ordered autograd {grid}] largest difference to the atomic form's table gradient {close:.3e} (largest entry {float(grads[0].abs().max()):.3e})")
    assert close <= 1e-5 * float(grads[0].abs().max())
    s = enc._scalings_on(q.device)
    kw = dict(grid=grid)
    qg = q.clone().requires_grad_()
    hashgrid.hash_encode(qg, enc.hash_table, s, 10, table_grad="ordered", **kw).backward(g)
    qa = q.clone().requires_grad_()
    hashgrid.hash_encode(qa, enc.hash_table, s, 10, **kw).backward(g)
    assert torch.equal(bits(qg.grad), bits(qa.grad))
    empty = hashgrid.hash_encode(torch.empty(0, 3, device=gpu), enc.hash_table, s, 10, table_grad="ordered", **kw)
    enc.hash_table.grad = None
    empty.sum().backward()
    assert empty.shape == (0, 10) and float(enc.hash_table.grad.abs().sum()) == 0.0
    with pytest.raises(ValueError, match="table_grad"):
        hashgrid.hash_encode(q, enc.hash_table, s, 10, table_grad="nope", **kw)
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        hashgrid.hash_encode(q.cpu(), enc.hash_table.detach().cpu(), s.cpu(), 10, table_grad="ordered", **kw)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _scene(gpu):
    from signerf_amd import Cameras, SIGNeRFDataManager, SIGNeRFDataManagerConfig, scene

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_trained_scene as mts

    H = W = 32
    cams = Cameras(scene.benchmark_cameras(4)[:, :3], 40.0, 40.0, W / 2, H / 2, W, H).to(gpu)
    images = []
    for i in range(4):
        rb = cams.generate_rays(camera_indices=i)
        rgb, _, _ = mts.analytic_image(rb.origins.cpu().reshape(-1, 3), rb.directions.cpu().reshape(-1, 3))
        images.append((rgb.reshape(H, W, 3) * 255.0).round().to(torch.uint8))
    images = torch.stack(images).to(gpu)

    def manager():
        return SIGNeRFDataManager(SIGNeRFDataManagerConfig(train_num_rays_per_batch=1024), cams, images,
                                  generator=torch.Generator(device=gpu).manual_seed(0))

    every = torch.stack(torch.meshgrid(torch.arange(4), torch.arange(H), torch.arange(W), indexing="ij"), -1).reshape(-1, 3).to(gpu)
    return manager, every


def _train(gpu, manager, steps, **kw):
    """The analytic-scene loop of tests/test_gpu_trainer.py (4 cameras of 32 x 32, tables of 2^10 rows, (16, 8, 8) samples) over HipAdam, from
    one seed.  -> (model, optimiser, data manager)"""
    from signerf_amd.optimizers import HipAdam

    torch.manual_seed(0)
    torch.cuda.manual_seed_all(0)
    cfg = small_config(training_forward=True, training_mlp="hip", training_hashgrid_grad="ordered", use_lpips=False, log2_hashmap_size=10,
                       num_proposal_samples_per_ray=(16, 8), num_nerf_samples_per_ray=8, num_train_data=4, camera_optimizer_mode="off",
                       proposal_net_args_list=[{"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 128, "use_linear": False},
                                               {"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 256, "use_linear": False}], **kw)
    model = cfg.setup().to(gpu)
    model.train()
    assert all(m.table_grad == "ordered" for m in model.modules() if isinstance(m, HashEncoding))
    dm = manager()
    opt = HipAdam([p for p in model.parameters() if p.numel()], lr=1e-2, eps=1e-15)
    for step in range(steps):
        model.set_training_step(step)
        bundle, batch = dm.next_train(step)
        out = model(bundle)
        loss = sum(model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch)).values())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return model, opt, dm


@pytest.mark.parametrize("kw", [dict(), dict(implementation="tcnn", training_tcnn=True)], ids=["torch", "tcnn"])
def test_two_training_runs_from_one_seed_are_bit_identical(gpu, kw):
    manager, every = _scene(gpu)
    runs = []
    for _ in range(2):
        model, opt, _ = _train(gpu, manager, 10, **kw)
        state = {n: p.detach().clone() for n, p in model.named_parameters()}
        moments = {(n, k): opt.state[p][k].clone() for n, p in model.named_parameters() if p in opt.state for k in ("exp_avg", "exp_avg_sq")}
        runs.append((state, moments))
    diff_p = [n for n in runs[0][0] if not torch.equal(bits(runs[0][0][n]), bits(runs[1][0][n]))]
    diff_m = [k for k in runs[0][1] if not torch.equal(bits(runs[0][1][k]), bits(runs[1][1][k]))]
    print(f"\n[ordered model {kw.get('implementation', 'torch')}] 10 steps twice from one seed: {len(runs[0][0])} parameters, {len(runs[0][1])} Adam moments; "
          f"parameters that differ {diff_p}, moments that differ {diff_m}")
    assert len(runs[0][1]) >= 2 * 3 and not diff_p and not diff_m


@pytest.mark.parametrize("kw", [dict(), dict(implementation="tcnn", training_tcnn=True)], ids=["torch", "tcnn"])
def test_the_model_fits_the_analytic_scene_with_the_ordered_gradient(gpu, kw):
    manager, every = _scene(gpu)
    model, _, dm = _train(gpu, manager, 0, **kw)
    all_rays, all_pixels = dm.train_ray_generator(every)

    def whole_loss(m):
        with torch.no_grad():
            return float(m.get_loss_dict(m(all_rays), {"image": all_pixels})["rgb_loss"])

    first = whole_loss(model)
    model, _, _ = _train(gpu, manager, 60, **kw)
    final = whole_loss(model)
    print(f"\n[ordered model fit {kw.get('implementation', 'torch')}] rgb loss {first:.5f} -> {final:.5f} ({final / first:.3f} of the initial)")
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert final < 0.5 * first
