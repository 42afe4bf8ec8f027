"""The per-ray normal terms on the GPU (signerf_amd/train_normals.py over csrc/sn_normal_losses.h) against the fp64 restatement of
tests/train_normals_oracle.py: nerfstudio's orientation and pred-normal losses and the rendered normals, forward and backward.

Gate (tests/hashgrid_oracle.gate, the project's, factor 2): max |kernel - ref64| <= 2 x max |restatement32 - ref64| + 1 ulp of the
largest output; the kernels sum in fp64 and round once, so their error is that last rounding.  Figures are printed before they are
asserted (pytest -s shows them)."""
import pytest
import torch

import hashgrid_oracle as ho
import train_normals_oracle as to
from signerf_amd import _lib, train_normals

pytestmark = pytest.mark.gpu
D = torch.float64
SHAPES = [(37, 11), (1, 1), (3, 64), (2, 65), (2, 1024), (0, 8)]
NAMES = ("orientation", "pred_normal", "rendered normals", "rendered pred_normals")


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(gpu):
    """A device error ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize(gpu)
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _gate(name, got, ref64, ref32):
    if ref64.numel() == 0:
        assert got.shape == ref64.shape
        return
    ok, e_hip, e_ref, limit = ho.gate(got.detach().cpu(), ref64, ref32)
    print(f"{name}: e_hip {e_hip:.2e} e_ref32 {e_ref:.2e} limit {limit:.2e}")
    assert got.shape == ref64.shape and got.dtype == torch.float32 and ok, f"{name}: {e_hip:.3e} > {limit:.3e}"


def _call(gpu, w, n, p, d, requires_grad=True):
    pg = p.to(gpu).requires_grad_(requires_grad)
    return pg, train_normals._normal_terms(w.to(gpu)[..., None], n.to(gpu), pg, d.to(gpu))


@pytest.mark.parametrize("R,S", SHAPES)
def test_forward_and_backward_against_fp64(gpu, R, S):
    w, n, p, d = to.ray_inputs(R, S, seed=100 * R + S)
    pg, got = _call(gpu, w, n, p, d)
    ref64, ref32 = to.terms(w, n, p, d, D), to.terms(w, n, p, d, torch.float32)
    for name, g, r64, r32 in zip(NAMES, got, ref64, ref32):
        _gate(f"R={R} S={S} {name}", g, r64, r32)
    assert [t.requires_grad for t in got] == [False, True, False, False]
    lo_, pn_ = train_normals.normal_losses(w.to(gpu)[..., None], n.to(gpu), p.to(gpu), d.to(gpu))
    assert torch.equal(lo_, got[0]) and torch.equal(pn_, got[1].detach())
    assert torch.equal(train_normals.render_normals(w.to(gpu)[..., None], n.to(gpu)), got[2])
    # the gradient: autograd of the torch formula, for a g that differs from ray to ray
    g = torch.linspace(-1.0, 2.0, max(R, 1))[:R]
    wg, ng = w.to(gpu)[..., None].requires_grad_(), n.to(gpu).requires_grad_()
    _, pred, _, _ = train_normals._normal_terms(wg, ng, pg, d.to(gpu))
    pred.backward(g.to(gpu))
    assert wg.grad is None and ng.grad is None                 # detached in nerfacto's call: no gradient
    _gate(f"R={R} S={S} grad_pred_normals", pg.grad, to.pred_normal_grad(w, n, p, g, D), to.pred_normal_grad(w, n, p, g, torch.float32))


def test_facing_the_camera_facing_away_and_a_nan_normal(gpu):
    """Rays whose normals all face the camera (n . (-d) >= 0): orientation exactly 0.  Rays whose normals all face away: every sample
    counts.  One NaN normal: torch.fmin hands back the 0, so the sample contributes w * 0 to the orientation term (and a NaN to the
    others) -- held against torch.fmin on the GPU itself, and the other rays are untouched."""
    R, S = 6, 65
    w, n, p, d = to.ray_inputs(R, S, seed=5)
    w = w.clamp_min(1e-3)                                       # every sample counts
    toward = torch.sign((n * (-d)[:, None, :]).sum(-1, keepdim=True))
    n[:2] = n[:2] * toward[:2]                                  # rays 0, 1: n . (-d) >= 0 everywhere
    n[2:4] = -n[2:4] * toward[2:4]                              # rays 2, 3: n . (-d) <= 0 everywhere
    n[5, 17, 1] = float("nan")
    _, got = _call(gpu, w, n, p, d, requires_grad=False)
    ref64, ref32 = to.terms(w, n, p, d, D), to.terms(w, n, p, d, torch.float32)
    assert bool((got[0][:2] == 0).all()) and bool((got[0][2:4] > 0).all())
    on_gpu = to.orientation_loss(w.to(gpu), n.to(gpu), d.to(gpu))                  # torch.fmin on the device
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(on_gpu).all()) and bool(torch.isfinite(ref64[0]).all())
    _gate("orientation with a NaN normal", got[0], ref64[0], ref32[0])
    assert float((got[0] - on_gpu).abs().max()) <= 2 * float((ref32[0].double() - ref64[0]).abs().max()) + 2.0 ** -23 * float(ref64[0].max())
    for name, g, r64, r32 in zip(NAMES[1:], got[1:], ref64[1:], ref32[1:]):
        poisoned = torch.isnan(r64).reshape(R, -1).any(-1)
        assert poisoned.tolist() == ([False] * 5 + [True] if name != "rendered pred_normals" else [False] * 6)
        assert torch.equal(torch.isnan(g.cpu()), torch.isnan(r64))
        _gate(name, g[:5], r64[:5], r32[:5])


def test_two_calls_return_equal_bits(gpu):
    w, n, p, d = to.ray_inputs(37, 130, seed=9)
    a = _call(gpu, w, n, p, d)
    b = _call(gpu, w, n, p, d)
    g = torch.linspace(0.5, 1.5, 37, device=gpu)
    a[1][1].backward(g)
    b[1][1].backward(g)
    for x, y in list(zip(a[1], b[1])) + [(a[0].grad, b[0].grad)]:
        assert torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32))


def test_entry_points_refuse_what_the_family_refuses(gpu):
    lib = _lib.load()
    t = torch.zeros(64, device=gpu)
    P = t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.sn_loss_normals_forward(P, P, P, P, 2, 0, P, P, P, P, st) == _lib.SN_ERR_INVALID          # S out of range
    assert lib.sn_loss_normals_forward(P, P, P, P, 2, 1025, P, P, P, P, st) == _lib.SN_ERR_INVALID
    assert lib.sn_loss_normals_forward(P, P, None, P, 2, 4, P, P, P, P, st) == _lib.SN_ERR_INVALID       # pred_normal without pred_normals
    assert lib.sn_loss_normals_forward(P, P, P, None, 2, 4, P, P, P, P, st) == _lib.SN_ERR_INVALID       # orientation without directions
    assert lib.sn_loss_normals_forward(P, P, P, P, 2, 4, None, None, None, None, st) == _lib.SN_ERR_INVALID
    assert b"sn_loss_normals_forward" in lib.sn_last_error(None)
    assert lib.sn_loss_normals_backward(P, P, None, 2, 4, P, st) == _lib.SN_ERR_INVALID
    assert lib.sn_loss_normals_forward(None, None, None, None, 0, 4, None, None, None, None, st) == _lib.SN_OK
    assert lib.sn_loss_normals_backward(None, None, None, 0, 4, None, st) == _lib.SN_OK
    torch.cuda.synchronize(gpu)
    assert bool((t == 0).all())
    # the Python entry points: shapes raise ValueError (after dtype and device)
    w, n, p, d = (x.to(gpu) for x in to.ray_inputs(3, 5, seed=0))
    w = w[..., None]
    with pytest.raises(ValueError, match="weights"):
        train_normals.normal_losses(w[..., 0], n, p, d)
    with pytest.raises(ValueError, match="pred_normals"):
        train_normals.normal_losses(w, n, p[:, :4], d)
    with pytest.raises(ValueError, match="directions"):
        train_normals.normal_losses(w, n, p, d[:2])
    with pytest.raises(ValueError, match="normals"):
        train_normals.render_normals(w, n[..., :2])
    with pytest.raises(TypeError, match="fp32"):
        train_normals.normal_losses(w, n.double(), p.cpu(), d)              # (dtype before device)
