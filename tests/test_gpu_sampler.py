"""Training-mode proposal sampling on the GPU (signerf_amd/samplers.py over csrc/sn_sampler.h) against tests/sampler_oracle.py on the CPU,
the training paths of the fields against the HIP stage with the literal torch-path arithmetic, ``get_training_outputs`` through the
losses and ``backward()``, and a short end-to-end fit.

The gate of the resampled spacing bins: with ``e_hip`` the max-abs error of the kernel against the fp64 restatement and ``e_ref32`` that
of the same restatement run in fp32 on the CPU, ``e_hip <= 2 e_ref32 + 1 ulp of the largest output``; both figures are printed per case
(pytest -s shows them).  Everything downstream of the spacing bins -- and the whole initial sampler -- is compared bit for bit."""
import ctypes as C
import functools
import itertools

import pytest
import torch

import sampler_oracle as so
from helpers import small_config
from signerf_amd import RayBundle, RaySamples, _lib, samplers

pytestmark = pytest.mark.gpu
D = torch.float64
RS = (1, 63, 65, 257)
LEVELS = [(1, 1), (2, 257), (65, 64), (256, 96), (96, 48), (8, 1024), (1024, 8)]
ANNEALS = (0.0, 0.35, 1.0)
PLANES = (0.05, 1000.0)


def _ulp(x: float) -> float:
    t = torch.tensor(abs(x), dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(float("inf"))) - t)


def same(a, b) -> bool:
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype == torch.float32:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return a.shape == b.shape and torch.equal(a, b)


def _combos(R):
    """(single_jitter, mode, per_ray): the full cross at R = 257; elsewhere three combinations that rotate with R, two of them
    complements of each other, so that every value of every factor is run at every R."""
    full = list(itertools.product((True, False), so.MODES, (True, False)))
    i = R % 8
    return full if R == 257 else [full[i], full[i ^ 7], full[(i + 3) % 8]]


@functools.lru_cache(maxsize=None)
def _rays(R, mode):
    return so.rays(R, seed=R, far_out=(mode == "uniform"))


def _bundle(gpu, R, mode, per_ray):
    o, d, nears, fars = _rays(R, mode)
    return RayBundle(origins=o.to(gpu), directions=d.to(gpu), pixel_area=torch.ones(R, 1, device=gpu),
                     camera_indices=torch.arange(R, device=gpu)[:, None] % 4,
                     nears=nears[:, None].to(gpu) if per_ray else None, fars=fars[:, None].to(gpu) if per_ray else None)


def _near_far(R, mode, per_ray):
    o, d, nears, fars = _rays(R, mode)
    return (nears, fars) if per_ray else (torch.full((R,), PLANES[0]), torch.full((R,), PLANES[1]))


def _check_downstream(rs, R, S, mode, per_ray):
    """Euclidean bins, deltas, positions, q and selector equal the fp32 restatement applied to the kernel's OWN spacing bins, bit for bit
    (this keeps the ill-conditioned s^-1 near far_plane out of the comparison); and the RaySamples has nerfstudio's shapes."""
    o, d, _, _ = _rays(R, mode)
    nears, fars = _near_far(R, mode, per_ray)
    sb = rs.spacing_bins.cpu()
    eb = so.euclid(sb, nears, fars, mode)
    assert same(rs.euclid_bins, eb)
    deltas, pos, q, sel = so.samples(eb, o, d)
    assert same(rs.deltas[..., 0], deltas) and same(rs.positions, pos) and same(rs.q, q) and same(rs.selector, sel)
    fr = rs.frustums
    assert fr.origins.shape == fr.directions.shape == (R, S, 3) and fr.starts.shape == fr.ends.shape == fr.pixel_area.shape == (R, S, 1)
    assert rs.deltas.shape == rs.spacing_starts.shape == rs.spacing_ends.shape == rs.camera_indices.shape == (R, S, 1)
    assert same(fr.starts[..., 0], eb[:, :-1]) and same(fr.ends[..., 0], eb[:, 1:]) and same(rs.spacing_starts[..., 0], sb[:, :-1])
    assert same(rs.spacing_ends[..., 0], sb[:, 1:]) and same(fr.origins[:, 0], o) and same(fr.directions[:, -1], d)
    return sel


# ---- the initial sampler -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 8, 65, 96, 256, 1024])
def test_initial_sampler_equals_the_fp32_restatement_bit_for_bit(gpu, N):
    dropped = 0
    for R in RS:
        for single, mode, per_ray in _combos(R):
            rand = so.uniforms(R, N + 1, single, seed=N)
            rs, used = samplers.sample_initial(_bundle(gpu, R, mode, per_ray), N, spacing_mode=mode, single_jitter=single, near_plane=PLANES[0],
                                               far_plane=PLANES[1], rand=rand.to(gpu), return_rand=True)
            assert same(used, rand)
            want = so.initial_bins(torch.linspace(0.0, 1.0, N + 1), rand)
            assert same(rs.spacing_bins, want.expand(R, N + 1)), (R, single, mode, per_ray)
            sel = _check_downstream(rs, R, N, mode, per_ray)
            dropped += int((~sel).sum())
    assert dropped > 0          # the uniform sampler's far rays leave the selector


# ---- the PDF resampler ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pdf_case(R, N, M, single, anneal):
    bins, w = so.previous_level(R, N, seed=N + M)
    rand = so.uniforms(R, M + 1, single, seed=M)
    grid = so.u_grid(M)
    ref64, _, _ = so.pdf_bins(bins, w, so.train_u(grid, rand, D), anneal=anneal, dtype=D)
    ref32, _, _ = so.pdf_bins(bins, w, so.train_u(grid, rand), anneal=anneal)
    return bins, w, rand, ref64, ref32


def _previous(gpu, bins):
    return RaySamples(frustums=None, spacing_starts=bins[:, :-1, None].to(gpu), spacing_ends=bins[:, 1:, None].to(gpu))


@pytest.mark.parametrize("N,M", LEVELS)
def test_pdf_sampler_against_the_fp64_restatement(gpu, N, M):
    worst = (0.0, 0.0)
    for R in RS:
        for k, (single, mode, per_ray) in enumerate(_combos(R)):
            for anneal in (ANNEALS if R == 257 else (ANNEALS[k % 3],)):
                bins, w, rand, ref64, ref32 = _pdf_case(R, N, M, single, anneal)
                rs, used = samplers.sample_pdf(_bundle(gpu, R, mode, per_ray), _previous(gpu, bins), w[..., None].to(gpu), M, anneal=anneal,
                                               spacing_mode=mode, single_jitter=single, near_plane=PLANES[0], far_plane=PLANES[1],
                                               rand=rand.to(gpu), return_rand=True)
                assert same(used, rand)
                hip = rs.spacing_bins.double().cpu()
                e_hip, e_ref = float((hip - ref64).abs().max()), float((ref32.double() - ref64).abs().max())
                ulp = _ulp(float(ref64.abs().max()))
                worst = max(worst, (e_hip, e_ref))
                tag = f"pdf[{N}->{M}, R={R}, {'single' if single else 'per-edge'}, anneal={anneal}, {mode}]"
                assert torch.isfinite(hip).all(), tag
                assert e_hip <= 2 * e_ref + ulp, (tag, e_hip, e_ref)
                assert so.decreasing_pairs(rs.spacing_bins.cpu()) == 0, tag
                assert bool((hip >= bins[:, :1].double()).all()) and bool((hip <= bins[:, -1:].double()).all()), tag
                _check_downstream(rs, R, M, mode, per_ray)
    print(f"pdf[{N}->{M}]: worst e_hip {worst[0]:.3e} beside e_ref32 {worst[1]:.3e}  ulp(1) {_ulp(1.0):.3e}")


# ---- random numbers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single", [True, False], ids=["single", "per-edge"])
def test_seeded_calls_use_the_philox_restatement_and_replay_bit_for_bit(gpu, single):
    R, N, M, seed, offset = 257, 96, 48, 0x0123456789ABCDEF, (7 << 32) | 123
    b = _bundle(gpu, R, "piecewise", True)
    bins, w = so.previous_level(R, N, seed=5)
    fields = ("spacing_bins", "euclid_bins", "deltas", "positions", "q", "selector")

    def initial(**kw):
        return samplers.sample_initial(b, N, single_jitter=single, return_rand=True, **kw)

    def pdf(**kw):
        return samplers.sample_pdf(b, _previous(gpu, bins), w[..., None].to(gpu), M, anneal=0.35, single_jitter=single, return_rand=True, **kw)

    for call, S in ((initial, N), (pdf, M)):
        rs, used = call(seed=seed, offset=offset)
        assert used.shape == ((R,) if single else (R, S + 1))          # one number per ray under single jitter
        assert same(used, so.philox_uniform(R, S + 1, seed, offset, single))
        replay, again = call(rand=used)
        twin, _ = call(seed=seed, offset=offset)
        other, other_used = call(seed=seed, offset=offset + 1)
        assert same(again, used)
        for f in fields:
            assert same(getattr(replay, f), getattr(rs, f)) and same(getattr(twin, f), getattr(rs, f)), f
        assert not same(other_used, used) and not same(other.spacing_bins, rs.spacing_bins)


# ---- isolation -----------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_ray_changes_only_its_own_rows(gpu):
    R, N, M = 65, 96, 48
    o, d, nears, fars = (t.clone() for t in so.rays(R, seed=9))
    bins, w = so.previous_level(R, N, seed=9)
    rand = so.uniforms(R, M + 1, False, seed=9)
    bad = [3, 17, 40, 64]

    def run(o, d, nears, fars, w):
        b = RayBundle(origins=o.to(gpu), directions=d.to(gpu), pixel_area=torch.ones(R, 1, device=gpu), nears=nears[:, None].to(gpu),
                      fars=fars[:, None].to(gpu))
        a = samplers.sample_initial(b, M, single_jitter=False, rand=rand.to(gpu))
        c = samplers.sample_pdf(b, _previous(gpu, bins), w[..., None].to(gpu), M, anneal=0.35, single_jitter=False, rand=rand.to(gpu))
        torch.cuda.synchronize()          # the call returns
        return a, c

    clean = run(o, d, nears, fars, w)
    o2, fars2, nears2, w2 = o.clone(), fars.clone(), nears.clone(), w.clone()
    o2[3, 1] = float("nan")
    fars2[17] = float("inf")
    w2[40, 5] = float("nan")
    nears2[64] = float("nan")
    w2[64] = float("inf")
    dirty = run(o2, d, nears2, fars2, w2)
    keep = torch.ones(R, dtype=torch.bool)
    keep[bad] = False
    for x, y in zip(clean, dirty):
        for f in ("spacing_bins", "euclid_bins", "deltas", "positions", "q", "selector"):
            assert same(getattr(x, f).cpu()[keep], getattr(y, f).cpu()[keep]), f
    assert torch.isnan(dirty[1].positions.cpu()[3, :, 1]).all() and torch.isnan(dirty[0].euclid_bins.cpu()[64]).all()


# ---- null outputs --------------------------------------------------------------------------------------------------------------------------
def test_null_outputs_are_not_written_and_zero_rays_succeed(gpu):
    R, N, M = 63, 65, 64
    o, d, nears, fars = (t.to(gpu) for t in so.rays(R, seed=2))
    bins, w = (t.to(gpu) for t in so.previous_level(R, N, seed=2))
    lib = _lib.load()
    base, grid = torch.linspace(0.0, 1.0, M + 1).to(gpu), so.u_grid(M).to(gpu)
    sizes = {"spacing_bins": R * (M + 1), "euclid_bins": R * (M + 1), "deltas": R * M, "positions": R * M * 3, "q": R * M * 3, "selector": R * M,
             "rand_out": R}
    GUARD = 64

    def call(kind, wanted, n_rays=R):
        bufs = {k: (torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=gpu) if k == "selector"
                    else torch.full((n + 2 * GUARD,), -777.0, device=gpu)) for k, n in sizes.items()}
        a = _lib.SnSamplerRays()
        a.n_samples, a.n_rays, a.origins, a.directions, a.nears, a.fars = M, n_rays, o.data_ptr(), d.data_ptr(), nears.data_ptr(), fars.data_ptr()
        a.single_jitter, a.seed, a.offset = 1, 11, 5
        for k in wanted:
            setattr(a, k, bufs[k].data_ptr() + GUARD * bufs[k].element_size())
        if kind == "initial":
            st = lib.sn_sampler_initial(C.byref(a), base.data_ptr(), _lib.current_stream())
        else:
            p = _lib.SnSamplerPdf()
            p.n_in, p.spacing_bins, p.weights, p.u_grid, p.anneal, p.histogram_padding = N, bins.data_ptr(), w.data_ptr(), grid.data_ptr(), 1.0, 0.01
            st = lib.sn_sampler_pdf(C.byref(a), C.byref(p), _lib.current_stream())
        torch.cuda.synchronize()
        assert st == 0, lib.sn_last_error(None)
        return {k: v.cpu() for k, v in bufs.items()}

    for kind in ("initial", "pdf"):
        full = call(kind, list(sizes))
        for wanted in (["deltas"], ["selector", "rand_out"], ["q"], ["spacing_bins", "positions"], []):
            got = call(kind, wanted)
            for k, n in sizes.items():
                untouched = torch.full_like(got[k], 0x5A if k == "selector" else -777.0)
                if k in wanted:          # the asked-for output is the full call's, and its guard bands are intact
                    assert torch.equal(got[k], full[k]), (kind, wanted, k)
                    assert torch.equal(got[k][:GUARD], untouched[:GUARD]) and torch.equal(got[k][-GUARD:], untouched[-GUARD:])
                    assert not torch.equal(got[k], untouched)
                else:
                    assert torch.equal(got[k], untouched), (kind, wanted, k)
        none = call(kind, list(sizes), n_rays=0)
        assert all(torch.equal(v, torch.full_like(v, 0x5A if k == "selector" else -777.0)) for k, v in none.items())
    empty = RayBundle(origins=torch.zeros(0, 3, device=gpu), directions=torch.zeros(0, 3, device=gpu), pixel_area=torch.zeros(0, 1, device=gpu))
    rs = samplers.sample_initial(empty, 16)
    assert rs.frustums.starts.shape == (0, 16, 1) and rs.q.shape == (0, 16, 3)


# ---- the fields' training paths ------------------------------------------------------------------------------------------------------------
def _tiny_config(**kw):
    """tables of 2^10 rows, levels of (16, 8, 8) samples: the smallest nerfacto that still has every part."""
    from signerf_amd.config import NerfactoModelConfig

    base = dict(log2_hashmap_size=10, num_proposal_samples_per_ray=(16, 8), num_nerf_samples_per_ray=8, num_train_data=4,
                camera_optimizer_mode="off", training_forward=True,
                proposal_net_args_list=[{"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 128, "use_linear": False},
                                        {"hidden_dim": 16, "log2_hashmap_size": 10, "num_levels": 5, "max_res": 256, "use_linear": False}])
    base.update(kw)
    return NerfactoModelConfig(**base)


def test_training_paths_of_the_fields_match_the_hip_stage(gpu):
    """``forward_training(appearance="mean")`` and ``get_density_training`` against ``ops.field_forward(..., return_geo=True)`` in its
    literal torch-path arithmetic (precision "fp32"), under the gates tests/test_gpu_field_surface.py applies to that entry point --
    on a sampler's own samples (the kernel's q / selector) and on samples from elsewhere (torch-op positions, far ones included)."""
    from helpers import make_model
    from signerf_amd import FieldHeadNames, Frustums, ops

    cfg = small_config(precision="fp32")
    model, _ = make_model(cfg, gpu)
    R, S = 37, 11
    b = _bundle(gpu, R, "piecewise", True)
    from_sampler = samplers.sample_initial(b, S, single_jitter=False, seed=3)
    g = torch.Generator().manual_seed(0)
    o = (torch.rand(R, 1, 3, generator=g) - 0.5).expand(R, S, 3).contiguous()
    d = torch.nn.functional.normalize(torch.randn(R, 1, 3, generator=g), dim=-1).expand(R, S, 3).contiguous()
    bins = torch.cumsum(torch.rand(R, S + 1, 1, generator=g) * 0.4, dim=1)
    bins[:3] *= 30.0
    elsewhere = RaySamples(Frustums(o.to(gpu), d.to(gpu), bins[:, :-1].to(gpu), bins[:, 1:].to(gpu), torch.ones(R, S, 1, device=gpu)))
    for rs in (from_sampler, elsewhere):
        pos, dirs = rs.frustums.get_positions().reshape(-1, 3), rs.frustums.directions.reshape(-1, 3)
        rd, rrgb, rgeo = ops.field_forward(model, pos, dirs, return_geo=True)
        out = model.field.forward_training(rs, appearance="mean", return_geo=True)
        density, rgb, geo = out[FieldHeadNames.DENSITY], out[FieldHeadNames.RGB], out["geo"]
        assert density.shape == (R, S, 1) and rgb.shape == (R, S, 3) and geo.shape == (R, S, 15) and density.requires_grad and rgb.requires_grad
        e_d = float(((density.detach().reshape(-1) - rd).abs() / rd.clamp_min(1e-6)).max())
        scale = float(rgeo.abs().max())
        e_g, e_c = float((geo.detach().reshape(-1, 15) - rgeo).abs().max()), float((rgb.detach().reshape(-1, 3) - rrgb).abs().max())
        print(f"field training path: density rel {e_d:.2e}  geo {e_g:.2e} (scale {scale:.2f})  rgb {e_c:.2e}")
        assert e_d <= 1e-4 and e_g <= 2e-5 * max(scale, 1.0) and e_c <= 2e-5
        for i, net in enumerate(model.proposal_networks):
            ri, _ = ops.field_forward(model, pos, None, which=i)
            di = net.get_density_training(rs)
            assert di.shape == (R, S, 1) and di.requires_grad
            assert float(((di.detach().reshape(-1) - ri).abs() / ri.clamp_min(1e-6)).max()) <= 1e-4
    with pytest.raises(NotImplementedError):
        model.field.forward_training(from_sampler, compute_normals=True)
    with pytest.raises(ValueError, match="camera_indices"):
        model.field.forward_training(elsewhere, appearance="per_camera")


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def _train_batch(gpu, R=256, seed=0):
    o, d, _, _ = so.rays(R, seed=seed)
    g = torch.Generator().manual_seed(seed)
    b = RayBundle(origins=(0.4 * o).to(gpu), directions=d.to(gpu), pixel_area=torch.ones(R, 1, device=gpu),
                  camera_indices=torch.randint(0, 4, (R, 1), generator=g).to(gpu))
    return b, {"image": torch.rand(R, 3, generator=g).to(gpu)}


def test_training_outputs_feed_the_losses_and_backward(gpu):
    torch.manual_seed(0)
    cfg = _tiny_config()
    model = cfg.setup().to(gpu)
    model.train()
    assert model.get_training_callbacks() == []
    R = 256
    b, batch = _train_batch(gpu, R)

    def step(at):
        model.zero_grad(set_to_none=True)
        model.set_training_step(at)
        out = model(b)                                   # training_forward=True and train(): get_training_outputs
        metrics = model.get_metrics_dict(out, batch)
        losses_ = model.get_loss_dict(out, batch, metrics)
        assert set(losses_) == {"rgb_loss", "interlevel_loss", "distortion_loss"} and "distortion" in metrics and "psnr" in metrics
        sum(losses_.values()).backward()
        return out

    out = step(0)                                         # step < 10: the proposal networks are updated
    assert set(out) == {"rgb", "accumulation", "depth", "expected_depth", "weights_list", "ray_samples_list", "prop_depth_0", "prop_depth_1"}
    assert out["rgb"].shape == (R, 3) and out["rgb"].requires_grad
    for k in ("accumulation", "depth", "expected_depth", "prop_depth_0", "prop_depth_1"):
        assert out[k].shape == (R, 1) and torch.isfinite(out[k]).all(), k
    assert not out["depth"].requires_grad and not out["prop_depth_0"].requires_grad
    assert [w.shape for w in out["weights_list"]] == [(R, 16, 1), (R, 8, 1), (R, 8, 1)]
    assert [rs.frustums.starts.shape for rs in out["ray_samples_list"]] == [(R, 16, 1), (R, 8, 1), (R, 8, 1)]
    for rs in out["ray_samples_list"]:
        assert rs.spacing_starts.shape == rs.spacing_ends.shape == rs.deltas.shape and not rs.spacing_starts.requires_grad
    params = list(model.field.named_parameters()) + list(model.proposal_networks.named_parameters())
    assert len(params) >= 18
    for name, p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert all(float(p.grad.abs().max()) > 0 for n, p in params if n.endswith("hash_table"))
    sampler = model._training_sampler()
    assert sampler._anneal == 0.0 and sampler._calls == 1

    step(20)                                              # one step after an update, update_sched(20) = 1: no update
    assert sampler._anneal == pytest.approx(samplers.anneal_at(20, 10.0, 1000)) and sampler._calls == 2
    assert all(p.grad is None for p in model.proposal_networks.parameters())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.field.parameters())

    # eval mode, and training_forward=False in either mode: the eval render, as before
    model.eval()
    ev = model(b)
    assert "weights_list" not in ev and ev["rgb"].shape == (R, 3)
    model.train()
    model.config.training_forward = False
    assert "weights_list" not in model(b)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def test_a_training_loop_fits_an_analytic_scene(gpu):
    """4 cameras of 32 x 32 of the analytic scene of tools/make_trained_scene.py (its density and colour functions, sphere-traced), 60 Adam
    steps of SIGNeRFDataManager.next_train -> model(ray_bundle) -> get_loss_dict -> backward on the smallest nerfacto: the rgb loss over
    all 4096 pixels ends below half of what it was before the first step (the ratio the hash-grid fit test gates at)."""
    import os
    import sys

    from helpers import ROOT
    from signerf_amd import Cameras, SIGNeRFDataManager, SIGNeRFDataManagerConfig, scene

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_trained_scene as mts

    torch.manual_seed(0)
    H = W = 32
    cams = Cameras(scene.benchmark_cameras(4)[:, :3], 40.0, 40.0, W / 2, H / 2, W, H).to(gpu)
    images = []
    for i in range(4):
        rb = cams.generate_rays(camera_indices=i)
        rgb, _, _ = mts.analytic_image(rb.origins.cpu().reshape(-1, 3), rb.directions.cpu().reshape(-1, 3))
        images.append((rgb.reshape(H, W, 3) * 255.0).round().to(torch.uint8))
    images = torch.stack(images).to(gpu)
    dm = SIGNeRFDataManager(SIGNeRFDataManagerConfig(train_num_rays_per_batch=1024), cams, images,
                            generator=torch.Generator(device=gpu).manual_seed(0))
    model = _tiny_config().setup().to(gpu)
    model.train()
    every = torch.stack(torch.meshgrid(torch.arange(4), torch.arange(H), torch.arange(W), indexing="ij"), -1).reshape(-1, 3).to(gpu)
    all_rays, all_pixels = dm.train_ray_generator(every)

    def whole_loss():
        with torch.no_grad():
            return float(model.get_loss_dict(model(all_rays), {"image": all_pixels})["rgb_loss"])

    first = whole_loss()
    opt = torch.optim.Adam([p for p in model.parameters() if p.numel()], lr=1e-2, eps=1e-15)
    for step in range(60):
        model.set_training_step(step)
        bundle, batch = dm.next_train(step)
        out = model(bundle)
        loss = sum(model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch)).values())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    final = whole_loss()
    print(f"\n[training fit] rgb loss {first:.5f} -> {final:.5f} ({final / first:.3f} of the initial)")
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert final < 0.5 * first
    model.mark_weights_dirty()                            # the optimizer wrote the parameters in place: the next eval render re-uploads them
    model.eval()
    assert torch.isfinite(model(all_rays.get_row_major_sliced_ray_bundle(0, 64))["rgb"]).all()
