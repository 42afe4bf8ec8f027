"""Training back half on the GPU (signerf_amd/losses.py over csrc/sn_losses.h): forward and backward of compositing, the distortion loss
and the interlevel loss against the fp64 restatement tests/loss_oracle.py on the CPU.

The gate of every comparison: with ``e_hip`` the max-abs error of the HIP result against fp64 and ``e_ref32`` that of the same restatement
run in fp32 on the CPU, ``e_hip <= 2 e_ref32 + 1 ulp of the largest output``.  Both figures are printed per case (pytest -s shows them)."""
import functools

import pytest
import torch

import loss_oracle as lo
from helpers import small_config
from signerf_amd import RaySamples, _lib, losses

pytestmark = pytest.mark.gpu
D = torch.float64

SHAPES = [(R, S) for R in (1, 63, 65, 257) for S in (1, 2, 47, 64, 65, 256)] + [(3, 1024)]
LEVELS = [(R, S, P) for R in (1, 63, 65, 257) for (S, P) in ((1, 1), (48, 96), (48, 256), (65, 64), (8, 1024))]


def _ulp(x: float) -> float:
    t = torch.tensor(abs(x), dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(float("inf"))) - t)


def gate(name, hip, ref64, ref32):
    hip, ref32 = hip.detach().double().cpu().reshape(ref64.shape), ref32.detach().double().reshape(ref64.shape)
    e_hip = float((hip - ref64).abs().max()) if ref64.numel() else 0.0
    e_ref = float((ref32 - ref64).abs().max()) if ref64.numel() else 0.0
    ulp = _ulp(float(ref64.abs().max())) if ref64.numel() else 0.0
    print(f"{name}: e_hip {e_hip:.3e}  e_ref32 {e_ref:.3e}  ulp(max) {ulp:.3e}  ratio {e_hip / max(e_ref, 1e-300):.3g}")
    assert torch.isfinite(hip).all()
    assert e_hip <= 2 * e_ref + ulp, name
    return e_hip, e_ref


def _f(x) -> float:
    return float(x.detach())


def _upstream(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- compositing ---------------------------------------------------------------------------------------------------------------------------
def _composite_reference(dtype, deltas, density, colour, bg, gw, grgb, gacc):
    density, colour = density.to(dtype, copy=True).requires_grad_(), colour.to(dtype, copy=True).requires_grad_()
    bgd = bg if isinstance(bg, str) else bg.to(dtype)
    w, rgb, acc = lo.composite(deltas.to(dtype), density, colour, bgd)
    gd, gc = torch.autograd.grad((w * gw.to(dtype)).sum() + (rgb * grgb.to(dtype)).sum() + (acc * gacc.to(dtype)).sum(), [density, colour])
    return [x.detach() for x in (w, rgb, acc, gd, gc)]


@functools.lru_cache(maxsize=None)
def _composite_case(R, S, constant_bg):
    deltas, density, colour = lo.composite_inputs(R, S, seed=1000 * R + S)
    bg = torch.tensor([0.25, 1.0, 0.6]) if constant_bg else "last_sample"
    ups = _upstream((R, S), 1), _upstream((R, 3), 2), _upstream((R, 1), 3)
    return (deltas, density, colour, bg, ups, _composite_reference(D, deltas, density, colour, bg, *ups),
            _composite_reference(torch.float32, deltas, density, colour, bg, *ups))


def _composite_hip(gpu, deltas, density, colour, bg, ups):
    dn, c = density.to(gpu).requires_grad_(), colour.to(gpu).requires_grad_()
    w, rgb, acc = losses.composite(dn[..., None], c, deltas.to(gpu)[..., None], bg if isinstance(bg, str) else bg.to(gpu))
    gw, grgb, gacc = (u.to(gpu) for u in ups)
    gd, gc = torch.autograd.grad((w[..., 0] * gw).sum() + (rgb * grgb).sum() + (acc * gacc).sum(), [dn, c])
    return [w[..., 0], rgb, acc, gd, gc]


@pytest.mark.parametrize("constant_bg", [False, True], ids=["last_sample", "constant"])
@pytest.mark.parametrize("R,S", SHAPES)
def test_composite_forward_and_backward(gpu, R, S, constant_bg):
    deltas, density, colour, bg, ups, ref64, ref32 = _composite_case(R, S, constant_bg)
    got = _composite_hip(gpu, deltas, density, colour, bg, ups)
    assert got[0].shape == (R, S) and got[1].shape == (R, 3) and got[2].shape == (R, 1)
    for name, h, a, b in zip(("weights", "rgb", "accumulation", "grad_density", "grad_colour"), got, ref64, ref32):
        gate(f"composite[{R}x{S},{'const' if constant_bg else 'last'}] {name}", h, a, b)


def test_get_weights_alone_and_its_gradient(gpu):
    R, S = 65, 47
    deltas, density, colour, bg, ups, ref64, ref32 = _composite_case(R, S, False)
    dn = density.to(gpu)[..., None].requires_grad_()
    w = losses.get_weights(deltas.to(gpu)[..., None], dn)
    assert w.shape == (R, S, 1)
    gate("get_weights", w, ref64[0], ref32[0])
    refs = []
    for dt in (D, torch.float32):
        x = density.to(dt, copy=True).requires_grad_()
        refs.append(torch.autograd.grad((lo.get_weights(deltas.to(dt), x) * ups[0].to(dt)).sum(), [x])[0])
    gd, = torch.autograd.grad((w[..., 0] * ups[0].to(gpu)).sum(), [dn])
    gate("get_weights grad_density", gd, refs[0], refs[1])
    # leading dimensions and a non-contiguous input
    strided = torch.stack([density, density + 1.0], dim=-1).to(gpu).reshape(5, 13, S, 2)[..., :1]
    assert not strided.is_contiguous()
    w2 = losses.get_weights(deltas.to(gpu).reshape(5, 13, S, 1), strided)
    assert w2.shape == (5, 13, S, 1) and torch.equal(w2.reshape(R, S, 1), w.detach())


# ---- distortion ----------------------------------------------------------------------------------------------------------------------------
def _distortion_reference(dtype, t, w, g):
    w = w.to(dtype, copy=True).requires_grad_()
    loss = lo.lossfun_distortion(t.to(dtype), w)
    return loss.detach(), torch.autograd.grad((loss * g.to(dtype)).sum(), [w])[0]


@functools.lru_cache(maxsize=None)
def _distortion_case(R, S, scale=1.0, offset=0.0):
    t, w = lo.histogram_inputs(R, S, seed=2000 * R + S, scale=scale, offset=offset)
    g = _upstream((R,), 4)
    return t, w, g, _distortion_reference(D, t, w, g), _distortion_reference(torch.float32, t, w, g)


def _distortion_hip(gpu, t, w, g):
    wg = w.to(gpu).requires_grad_()
    loss = losses.lossfun_distortion(t.to(gpu), wg)
    return loss, torch.autograd.grad((loss * g.to(gpu)).sum(), [wg])[0]


@pytest.mark.parametrize("R,S", SHAPES)
def test_distortion_forward_and_backward(gpu, R, S):
    t, w, g, ref64, ref32 = _distortion_case(R, S)
    loss, gw = _distortion_hip(gpu, t, w, g)
    assert loss.shape == (R,) and gw.shape == (R, S)
    gate(f"distortion[{R}x{S}] loss", loss, ref64[0], ref32[0])
    gate(f"distortion[{R}x{S}] grad_w", gw, ref64[1], ref32[1])


def test_distortion_with_large_close_edges(gpu):
    """Edges near 1000 and 1e-3 apart (a few fp32 ulps each): where a prefix-sum form would cancel; the pairwise form does not."""
    t, w, g, ref64, ref32 = _distortion_case(65, 47, scale=1e-3, offset=1000.0)
    loss, gw = _distortion_hip(gpu, t, w, g)
    gate("distortion[large close t] loss", loss, ref64[0], ref32[0])
    gate("distortion[large close t] grad_w", gw, ref64[1], ref32[1])


# ---- interlevel ----------------------------------------------------------------------------------------------------------------------------
def _outer_reference(dtype, t, w, t_env, w_env, g):
    w_env = w_env.to(dtype, copy=True).requires_grad_()
    loss = lo.lossfun_outer(t.to(dtype), w.to(dtype), t_env.to(dtype), w_env)
    return loss.detach(), torch.autograd.grad((loss * g.to(dtype)).sum(), [w_env])[0], lo.outer(t.to(dtype), t_env.to(dtype), w_env.detach())


@functools.lru_cache(maxsize=None)
def _outer_case(R, S, P, ties=False):
    if ties:
        t, w, t_env, w_env = lo.tie_inputs(R, S, P, seed=3000 * R + S)
    else:
        t, w = lo.histogram_inputs(R, S, seed=3000 * R + S)
        t_env, w_env = lo.histogram_inputs(R, P, seed=3000 * R + S + 1)
        w_env = (w_env * 0.7).contiguous()
    g = _upstream((R,), 5)
    return t, w, t_env, w_env, g, _outer_reference(D, t, w, t_env, w_env, g), _outer_reference(torch.float32, t, w, t_env, w_env, g)


def _outer_hip(gpu, t, w, t_env, w_env, g):
    we = w_env.to(gpu).requires_grad_()
    loss = losses.lossfun_outer(t.to(gpu), w.to(gpu), t_env.to(gpu), we)
    return loss, torch.autograd.grad((loss * g.to(gpu)).sum(), [we])[0], losses.outer(t.to(gpu), t_env.to(gpu), w_env.to(gpu))


@pytest.mark.parametrize("R,S,P", LEVELS)
def test_interlevel_forward_and_backward(gpu, R, S, P):
    t, w, t_env, w_env, g, ref64, ref32 = _outer_case(R, S, P)
    got = _outer_hip(gpu, t, w, t_env, w_env, g)
    assert got[0].shape == (R,) and got[1].shape == (R, P) and got[2].shape == (R, S)
    assert float(ref64[0].max()) > 0
    for name, h, a, b in zip(("loss", "grad_w_env", "w_outer"), got, ref64, ref32):
        gate(f"interlevel[{R}x{S},{P}] {name}", h, a, b)


@pytest.mark.parametrize("S,P", [(48, 96), (65, 64), (8, 1024), (3, 4)])
def test_interlevel_ties_and_zero_width_intervals(gpu, S, P):
    """The main edges are a subset of the envelope's (every deciding comparison is a tie) and both hold repeated edges: the indices are
    integer-exact by construction, so w_outer must meet the gate like everything else."""
    t, w, t_env, w_env, g, ref64, ref32 = _outer_case(33, S, P, ties=True)
    a, b = lo.outer_indices(t, t_env), lo.outer_indices(t.to(D), t_env.to(D))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    got = _outer_hip(gpu, t, w, t_env, w_env, g)
    for name, h, x, y in zip(("loss", "grad_w_env", "w_outer"), got, ref64, ref32):
        gate(f"interlevel ties[{S},{P}] {name}", h, x, y)


# ---- determinism, non-finite inputs, R = 0, refusals ---------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(gpu):
    deltas, density, colour, bg, ups, _, _ = _composite_case(257, 65, False)
    a, b = _composite_hip(gpu, deltas, density, colour, bg, ups), _composite_hip(gpu, deltas, density, colour, bg, ups)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    t, w, g, _, _ = _distortion_case(257, 65)
    a, b = _distortion_hip(gpu, t, w, g), _distortion_hip(gpu, t, w, g)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    case = _outer_case(257, 65, 64)[:5]
    a, b = _outer_hip(gpu, *case), _outer_hip(gpu, *case)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_non_finite_density_stays_in_its_ray(gpu):
    R, S = 65, 47
    deltas, density, colour, bg, ups, ref64, _ = _composite_case(R, S, False)
    bad = density.clone()
    bad[3, 10] = float("nan")
    bad[40, 20] = float("inf")
    bad[64, 0] = float("inf")
    rays = [3, 40, 64]
    keep = torch.ones(R, dtype=torch.bool)
    keep[rays] = False
    t = torch.sort(torch.rand(R, S + 1, generator=torch.Generator().manual_seed(9)), dim=-1).values.to(gpu)

    def run(dens):
        dn, c = dens.to(gpu).requires_grad_(), colour.to(gpu).requires_grad_()
        w, rgb, acc = losses.composite(dn[..., None], c, deltas.to(gpu)[..., None])
        dist = losses.lossfun_distortion(t, w[..., 0])
        gd, gc = torch.autograd.grad((w[..., 0] * ups[0].to(gpu)).sum() + (rgb * ups[1].to(gpu)).sum() + (acc * ups[2].to(gpu)).sum()
                                     + (dist * ups[2].to(gpu)[:, 0]).sum(), [dn, c])
        return [w[..., 0], rgb, acc, dist, gd, gc]

    clean, dirty = run(density), run(bad)
    # the corrupted rays: the oracle's forward weights (nan_to_num turns what the NaN reaches into 0)
    want64, want32 = lo.get_weights(deltas.to(D), bad.to(D)), lo.get_weights(deltas, bad)
    assert torch.isfinite(want64).all() and bool((want64[3, 10:] == 0).all()) and bool((want64[40, 21:] == 0).all())
    gate("non-finite rays: weights", dirty[0][rays], want64[rays], want32[rays])
    # every other ray: bit-identical outputs and gradients
    for name, x, y in zip(("weights", "rgb", "accumulation", "distortion", "grad_density", "grad_colour"), clean, dirty):
        assert torch.equal(x[keep.to(gpu)], y[keep.to(gpu)]), name


def test_zero_rays(gpu):
    S, P = 5, 7
    dn = torch.zeros(0, S, 1, device=gpu, requires_grad=True)
    c = torch.zeros(0, S, 3, device=gpu, requires_grad=True)
    w, rgb, acc = losses.composite(dn, c, torch.zeros(0, S, 1, device=gpu))
    assert w.shape == (0, S, 1) and rgb.shape == (0, 3) and acc.shape == (0, 1)
    assert losses.get_weights(torch.zeros(0, S, 1, device=gpu), dn).shape == (0, S, 1)
    wm = torch.zeros(0, S, device=gpu, requires_grad=True)
    we = torch.zeros(0, P, device=gpu, requires_grad=True)
    d = losses.lossfun_distortion(torch.zeros(0, S + 1, device=gpu), wm)
    o = losses.lossfun_outer(torch.zeros(0, S + 1, device=gpu), wm, torch.zeros(0, P + 1, device=gpu), we)
    assert d.shape == (0,) and o.shape == (0,)
    grads = torch.autograd.grad(w.sum() + rgb.sum() + acc.sum() + d.sum() + o.sum(), [dn, c, wm, we])
    assert [tuple(g.shape) for g in grads] == [(0, S, 1), (0, S, 3), (0, S), (0, P)]
    # the library itself: SN_OK, nothing launched, whatever the pointers
    lib = _lib.load()
    assert lib.sn_loss_composite_forward(None, None, None, None, 0, S, None, None, None, None) == 0
    assert lib.sn_loss_interlevel_backward(None, None, None, None, None, 0, S, P, None, None) == 0


def test_wrong_dtype_or_device_raise(gpu):
    x = torch.zeros(2, 4, 1, device=gpu)
    with pytest.raises(TypeError, match="fp32"):
        losses.get_weights(x.double(), x.double())
    with pytest.raises(TypeError, match="fp32"):
        losses.composite(x, torch.zeros(2, 4, 3, device=gpu, dtype=torch.float16), x)
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        losses.composite(x, torch.zeros(2, 4, 3), x)
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        losses.composite(x, torch.zeros(2, 4, 3, device=gpu), x, torch.zeros(3))
    with pytest.raises(TypeError, match="fp32"):
        losses.lossfun_distortion(torch.zeros(2, 5, device=gpu), torch.zeros(2, 4, device=gpu, dtype=torch.int32))
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        losses.lossfun_outer(torch.zeros(2, 5, device=gpu), torch.zeros(2, 4, device=gpu), torch.zeros(2, 9), torch.zeros(2, 8, device=gpu))
    with pytest.raises(ValueError, match="1..1024"):
        losses.lossfun_distortion(torch.zeros(2, 1026, device=gpu), torch.zeros(2, 1025, device=gpu))


# ---- the model's loss and metrics dicts ------------------------------------------------------------------------------------------------------
def _level(R, S, seed, gpu, scale=1.0):
    t, w = lo.histogram_inputs(R, S, seed)
    w = (w * scale).contiguous()
    rs = RaySamples(frustums=None, spacing_starts=t[:, :-1, None].to(gpu), spacing_ends=t[:, 1:, None].to(gpu))
    return t, w, rs, w[..., None].to(gpu).requires_grad_()


def _hand_made_outputs(gpu, R=32 * 32):
    levels = [_level(R, 24, 1, gpu, 0.7), _level(R, 12, 2, gpu, 0.7), _level(R, 6, 3, gpu)]
    g = torch.Generator().manual_seed(11)
    rgb, image = torch.rand(R, 3, generator=g), torch.rand(R, 3, generator=g)
    outputs = {"rgb": rgb.to(gpu).requires_grad_(), "weights_list": [lv[3] for lv in levels], "ray_samples_list": [lv[2] for lv in levels]}
    sd = [lv[0].to(D) for lv in levels]
    wl = [lv[1].to(D)[..., None] for lv in levels]
    want = {"interlevel": float(lo.interlevel_loss(wl, sd)), "distortion": float(lo.distortion_loss(wl, sd)),
            "mse": float(((rgb.to(D) - image.to(D)) ** 2).mean()), "l1": float((rgb.to(D) - image.to(D)).abs().mean())}
    return outputs, {"image": image}, want, rgb, image


class _StubLpips(torch.nn.Module):
    def forward(self, a, b):
        assert a.shape == b.shape and a.shape[1:] == (3, 32, 32) and float(a.detach().min()) >= -1 and float(a.detach().max()) <= 1
        return ((a - b) ** 2).mean()


def test_nerfacto_loss_and_metrics_dicts(gpu):
    from signerf_amd import NerfactoModelConfig

    cfg = small_config()
    model = NerfactoModelConfig(**{k: getattr(cfg, k) for k in ("log2_hashmap_size", "proposal_net_args_list")}).setup().to(gpu)
    assert model.config.interlevel_loss_mult == 1.0 and model.config.distortion_loss_mult == 0.002
    outputs, batch, want, _, _ = _hand_made_outputs(gpu)
    model.eval()
    metrics = model.get_metrics_dict(outputs, batch)
    assert set(metrics) == {"psnr"} and _f(metrics["psnr"]) == pytest.approx(-10 * torch.log10(torch.tensor(want["mse"])).item(), rel=1e-5)
    loss = model.get_loss_dict(outputs, batch, metrics)
    assert set(loss) == {"rgb_loss"} and _f(loss["rgb_loss"]) == pytest.approx(want["mse"], rel=1e-5)
    model.train()
    metrics = model.get_metrics_dict(outputs, batch)
    assert set(metrics) == {"psnr", "distortion"} and _f(metrics["distortion"]) == pytest.approx(want["distortion"], rel=1e-5)
    loss = model.get_loss_dict(outputs, batch, metrics)
    assert set(loss) == {"rgb_loss", "interlevel_loss", "distortion_loss"}
    assert _f(loss["interlevel_loss"]) == pytest.approx(want["interlevel"], rel=1e-5) and want["interlevel"] > 0
    assert _f(loss["distortion_loss"]) == pytest.approx(0.002 * want["distortion"], rel=1e-5)
    sum(loss.values()).backward()
    p0, p1, main = outputs["weights_list"]
    assert float(p0.grad.abs().max()) > 0 and float(p1.grad.abs().max()) > 0      # through the interlevel loss
    assert float(main.grad.abs().max()) > 0                                       # through the distortion loss (the interlevel loss detaches it)
    assert float(outputs["rgb"].grad.abs().max()) > 0
    # the gradient on the main weights is the distortion loss's alone
    t, w = lo.histogram_inputs(main.shape[0], 6, 3)
    wd = w.to(D).requires_grad_()
    ref, = torch.autograd.grad(0.002 * lo.lossfun_distortion(t.to(D), wd).mean(), [wd])
    assert float((main.grad[..., 0].double().cpu() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_signerf_loss_dict(gpu):
    outputs, batch, want, rgb, image = _hand_made_outputs(gpu)
    model = small_config(use_lpips=True).setup().to(gpu)
    assert (model.config.use_l1, model.config.patch_size, model.config.lpips_loss_mult) == (True, 32, 1.0)
    model.train()
    with pytest.raises(NotImplementedError, match="LPIPS weights are not shipped.*model.lpips"):
        model.get_loss_dict(outputs, batch, None)
    model.lpips = _StubLpips()
    loss = model.get_loss_dict(outputs, batch, model.get_metrics_dict(outputs, batch))
    # (predict_normals is set, but hand-made outputs hold no per-sample normal terms: those two losses are left out)
    assert set(loss) == {"rgb_loss", "lpips_loss", "interlevel_loss", "distortion_loss"}
    assert _f(loss["rgb_loss"]) == pytest.approx(want["l1"], rel=1e-5)
    a, b = ((x.view(-1, 32, 32, 3).permute(0, 3, 1, 2) * 2 - 1).clamp(-1, 1) for x in (rgb, image))
    assert _f(loss["lpips_loss"]) == pytest.approx(float(((a - b) ** 2).mean()), rel=1e-5)
    assert _f(loss["interlevel_loss"]) == pytest.approx(want["interlevel"], rel=1e-5)
    assert _f(loss["distortion_loss"]) == pytest.approx(0.002 * want["distortion"], rel=1e-5)
    sum(loss.values()).backward()
    assert all(float(w.grad.abs().max()) > 0 for w in outputs["weights_list"])
    model.eval()
    assert set(model.get_loss_dict(outputs, batch)) == {"rgb_loss", "lpips_loss"}
    mse = small_config(use_lpips=False, use_l1=False).setup().to(gpu)
    mse.eval()
    got = mse.get_loss_dict(outputs, batch)
    assert set(got) == {"rgb_loss"} and _f(got["rgb_loss"]) == pytest.approx(want["mse"], rel=1e-5)


# ---- a short optimisation ------------------------------------------------------------------------------------------------------------------
def test_fifty_adam_steps_halve_the_loss(gpu):
    R, S = 64, 16
    g = torch.Generator().manual_seed(0)
    t = torch.sort(torch.rand(R, S + 1, generator=g), dim=-1).values
    deltas = ((t[:, 1:] - t[:, :-1]) * 4.0)[..., None].to(gpu)
    t = t.to(gpu)
    density = (torch.rand(R, S, 1, generator=g) * 4 + 0.5).to(gpu).requires_grad_()
    colour = torch.rand(R, S, 3, generator=g).to(gpu).requires_grad_()
    target = torch.tensor([0.2, 0.6, 0.9], device=gpu).expand(R, 3)
    opt = torch.optim.Adam([density, colour], lr=0.02)
    history = []
    for _ in range(50):
        opt.zero_grad()
        w, rgb, _ = losses.composite(density, colour, deltas)
        loss = (rgb - target).abs().mean() + 0.002 * losses.lossfun_distortion(t, w[..., 0]).mean()
        loss.backward()
        assert float(density.grad.abs().max()) > 0 and float(colour.grad.abs().max()) > 0
        opt.step()
        history.append(_f(loss))
    print(f"adam: {history[0]:.4f} -> {history[-1]:.4f}")
    assert history[-1] < 0.5 * history[0]
