"""Training back half, CPU side: the restatement tests/loss_oracle.py against hand-computed closed forms, the hand-derived gradient formulas
(what csrc/sn_losses.h implements) against ``torch.autograd`` in fp64, ``searchsorted`` ties, and the companion C header
include/signerf_hip_losses.h against the binding, the library's exports and its argument refusals (in a child process: nothing is
launched).  No GPU."""
import math
import os

import pytest
import torch

import loss_oracle as lo
from abi_helpers import c99_probe, refusal_sweep
from helpers import ROOT
from signerf_amd import _lib

HEADER = os.path.join(ROOT, "include", "signerf_hip_losses.h")
D = torch.float64


# ---- closed forms --------------------------------------------------------------------------------------------------------------------------
def test_one_sample_closed_forms():
    delta, sigma = 0.25, 3.0
    c = torch.tensor([[[0.2, 0.5, 0.9]]], dtype=D)
    w, rgb, acc = lo.composite(torch.tensor([[delta]], dtype=D), torch.tensor([[sigma]], dtype=D), c)
    a = 1 - math.exp(-delta * sigma)
    assert float(w) == pytest.approx(a, rel=1e-15) and float(acc) == pytest.approx(a, rel=1e-15)
    assert torch.allclose(rgb, c[:, 0], rtol=1e-15)                      # last_sample: a c + c (1 - a) = c
    _, rgb, _ = lo.composite(torch.tensor([[delta]], dtype=D), torch.tensor([[sigma]], dtype=D), c, torch.tensor([1.0, 0.0, 0.5], dtype=D))
    assert rgb[0].tolist() == pytest.approx([a * 0.2 + (1 - a), a * 0.5, a * 0.9 + 0.5 * (1 - a)], rel=1e-14)
    # distortion of one interval: the pair term vanishes, (1/3) w^2 (t1 - t0) stays
    assert float(lo.lossfun_distortion(torch.tensor([[0.5, 0.75]], dtype=D), torch.tensor([[0.6]], dtype=D))) == pytest.approx(0.36 * 0.25 / 3, rel=1e-15)
    # one interval inside one envelope interval: max(w - w_env, 0)^2 / (w + eps)
    t, te = torch.tensor([[0.2, 0.4]], dtype=D), torch.tensor([[0.0, 1.0]], dtype=D)
    got = lo.lossfun_outer(t, torch.tensor([[0.8]], dtype=D), te, torch.tensor([[0.5]], dtype=D))
    assert float(got) == pytest.approx(0.3**2 / (0.8 + 1e-7), rel=1e-14)
    assert float(lo.lossfun_outer(t, torch.tensor([[0.3]], dtype=D), te, torch.tensor([[0.5]], dtype=D))) == 0.0


def test_two_equal_samples_closed_forms():
    delta, sigma = 0.5, 2.0
    a = 1 - math.exp(-delta * sigma)
    w = lo.get_weights(torch.full((1, 2), delta, dtype=D), torch.full((1, 2), sigma, dtype=D))
    assert w[0].tolist() == pytest.approx([a, a * (1 - a)], rel=1e-15)
    # two equal weights on [0, 1], [1, 2]: 2 w^2 |0.5 - 1.5| + (1/3) 2 w^2
    wv = 0.4
    got = lo.lossfun_distortion(torch.tensor([[0.0, 1.0, 2.0]], dtype=D), torch.full((1, 2), wv, dtype=D))
    assert float(got) == pytest.approx(2 * wv * wv + 2 * wv * wv / 3, rel=1e-15)
    g = lo.distortion_grad(torch.tensor([[0.0, 1.0, 2.0]], dtype=D), torch.full((1, 2), wv, dtype=D), torch.ones(1, dtype=D))
    assert g[0].tolist() == pytest.approx([2 * wv + 2 * wv / 3] * 2, rel=1e-15)


def test_outer_of_identical_and_of_empty_envelope():
    t = lo.histogram_inputs(5, 17, seed=3)[0].to(D)
    w = torch.randint(0, 16, (5, 17), generator=torch.Generator().manual_seed(3)).to(D) / 256    # dyadic: every partial sum is exact
    # a main level identical to its envelope: w_outer_i >= w_i (it adds the neighbours the interval touches) -> exactly 0
    assert torch.equal(lo.lossfun_outer(t, w, t, w), torch.zeros(5, dtype=D))
    lo_i, hi_i = lo.outer_indices(t, t)
    assert torch.equal(lo_i, torch.arange(17).expand(5, 17)) and torch.equal(hi_i, (torch.arange(17) + 1).clamp(max=16).expand(5, 17))
    # an envelope of zeros: w^2 / (w + eps), mean over the samples
    got = lo.lossfun_outer(t, w, t, torch.zeros_like(w))
    assert torch.allclose(got, (w * w / (w + 1e-7)).mean(-1), rtol=1e-14, atol=0)


# ---- the hand-derived gradients against autograd, fp64 -----------------------------------------------------------------------------------
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


@pytest.mark.parametrize("background", ["last_sample", "constant"])
@pytest.mark.parametrize("R,S", [(3, 1), (4, 2), (5, 47), (2, 130)])
def test_composite_gradient_formula_equals_autograd(R, S, background):
    g = torch.Generator().manual_seed(S)
    deltas = torch.rand(R, S, generator=g, dtype=D) * 0.2
    density = (10.0 ** (torch.rand(R, S, generator=g, dtype=D) * 3 - 2)).requires_grad_()
    colour = torch.rand(R, S, 3, generator=g, dtype=D).requires_grad_()
    bg = "last_sample" if background == "last_sample" else torch.tensor([0.3, 0.9, 0.1], dtype=D)
    gw, grgb, gacc = torch.randn(R, S, generator=g, dtype=D), torch.randn(R, 3, generator=g, dtype=D), torch.randn(R, 1, generator=g, dtype=D)
    w, rgb, acc = lo.composite(deltas, density, colour, bg)
    want_d, want_c = torch.autograd.grad((w * gw).sum() + (rgb * grgb).sum() + (acc * gacc).sum(), [density, colour])
    got_d, got_c = lo.composite_grad(deltas, density.detach(), colour.detach(), bg, gw, grgb, gacc)
    assert _rel(got_d, want_d) <= 1e-12 and _rel(got_c, want_c) <= 1e-12


@pytest.mark.parametrize("R,S", [(3, 1), (4, 2), (5, 47), (2, 130)])
def test_distortion_gradient_formula_equals_autograd(R, S):
    t, w = (x.to(D) for x in lo.histogram_inputs(R, S, seed=S))
    w.requires_grad_()
    g = torch.randn(R, generator=torch.Generator().manual_seed(1), dtype=D)
    want, = torch.autograd.grad((lo.lossfun_distortion(t, w) * g).sum(), [w])
    assert _rel(lo.distortion_grad(t, w.detach(), g), want) <= 1e-12


def _outer_case(R, S, P, seed, ties):
    if ties:
        return tuple(x.to(D) for x in lo.tie_inputs(R, S, P, seed))
    t, w = lo.histogram_inputs(R, S, seed)
    t_env, w_env = lo.histogram_inputs(R, P, seed + 1)
    return t.to(D), w.to(D), t_env.to(D), (w_env * 0.7).to(D)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("S,P", [(1, 1), (48, 96), (65, 64), (8, 200)])
def test_outer_gradient_formula_equals_autograd(S, P, ties):
    t, w, t_env, w_env = _outer_case(4, S, P, 10 + S, ties)
    w_env.requires_grad_()
    g = torch.randn(4, generator=torch.Generator().manual_seed(2), dtype=D)
    loss = lo.lossfun_outer(t, w, t_env, w_env)
    assert ties or S == 1 or float(loss.detach().max()) > 0
    want, = torch.autograd.grad((loss * g).sum(), [w_env])
    got = lo.outer_grad(t, w, t_env, w_env.detach(), g)
    assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300)


def test_searchsorted_ties_and_zero_width_intervals():
    """t a subset of t_env: the index rule on ties, worked by hand.  side="right" counts the edges <= the value, so an interval that starts ON
    an envelope edge starts in the interval to the right of it, and one that ends ON an edge reaches into the next one."""
    t_env = torch.tensor([[0.0, 1.0, 1.0, 2.0, 3.0]], dtype=D)     # P = 4, interval 1 has zero width
    t = torch.tensor([[0.0, 1.0, 1.0, 3.0]], dtype=D)              # S = 3, interval 1 has zero width
    lo_i, hi_i = lo.outer_indices(t, t_env)
    # starts t_env[:-1] = [0,1,1,2]: #(<= 0) - 1 = 0, #(<= 1) - 1 = 2, 2;  ends t_env[1:] = [1,1,2,3]: #(<= 1) = 2, 2, #(<= 3) = 4 -> 3
    assert lo_i.tolist() == [[0, 2, 2]] and hi_i.tolist() == [[2, 2, 3]]
    w_env = torch.tensor([[0.1, 0.2, 0.3, 0.4]], dtype=D)
    assert lo.outer(t, t_env, w_env)[0].tolist() == pytest.approx([0.6, 0.3, 0.7], rel=1e-15)
    # the construction the GPU test uses: every index is integer-exact and stays so in fp32
    t, w, t_env, w_env = lo.tie_inputs(6, 48, 96, seed=5)
    a = lo.outer_indices(t, t_env)
    b = lo.outer_indices(t.to(D), t_env.to(D))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert bool((t[:, 1:] == t[:, :-1]).any()) and bool((t_env[:, 1:] == t_env[:, :-1]).any())
    assert bool((a[1] >= a[0]).all()) and bool((a[0][:, 1:] >= a[0][:, :-1]).all()) and bool((a[1][:, 1:] >= a[1][:, :-1]).all())


# ---- the companion C header ------------------------------------------------------------------------------------------------------------
NAMES = ["sn_loss_composite_backward", "sn_loss_composite_forward", "sn_loss_distortion_backward", "sn_loss_distortion_forward",
         "sn_loss_interlevel_backward", "sn_loss_interlevel_forward", "sn_losses_abi_version"]


def test_losses_header_binding_and_exports_agree(built_lib):
    """(The header against the binding, the exports and build.HEADERS: tests/test_cabi.py, for every header.)"""
    assert sorted(_lib.header("losses").functions) == NAMES
    lib = _lib.load()
    assert lib.sn_losses_abi_version() == _lib.header("losses").version == 1
    blob = open(built_lib, "rb").read()
    for k in [n + "_kernel" for n in NAMES if n != "sn_losses_abi_version"]:
        assert 24 <= len(k) <= 99 and k.encode() in blob       # (names behind _Z23...: DESIGN.md §4 "Wide fields", "Kernel names")


def test_losses_header_compiles_as_c99(tmp_path):
    assert c99_probe(tmp_path, "signerf_hip_losses.h", "%d %d", "SN_LOSSES_ABI_VERSION, SN_LOSSES_MAX_SAMPLES") == ["1", "1024"]


_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
F = 0x1000   # never dereferenced: every call below is refused (or R == 0) before the device is touched
def done(st, name):
    msg = lib.sn_last_error(None)
    return "%d:%s" % (st, "text" if (st == 0 or (msg and name.encode() in msg)) else "notext")
def cf(deltas=F, density=F, colour=F, bg=N, R=4, S=8, w=F, rgb=F, acc=F):
    return done(lib.sn_loss_composite_forward(deltas, density, colour, bg, R, S, w, rgb, acc, N), "sn_loss_composite_forward")
def cb(deltas=F, density=F, colour=F, bg=N, R=4, S=8, gw=N, grgb=F, gacc=F, gd=F, gc=F):
    return done(lib.sn_loss_composite_backward(deltas, density, colour, bg, R, S, gw, grgb, gacc, gd, gc, N), "sn_loss_composite_backward")
def df(t=F, w=F, R=4, S=8, loss=F):
    return done(lib.sn_loss_distortion_forward(t, w, R, S, loss, N), "sn_loss_distortion_forward")
def db(t=F, w=F, g=F, R=4, S=8, gw=F):
    return done(lib.sn_loss_distortion_backward(t, w, g, R, S, gw, N), "sn_loss_distortion_backward")
def lf(t=F, w=F, te=F, we=F, R=4, S=8, P=16, loss=F, wo=N):
    return done(lib.sn_loss_interlevel_forward(t, w, te, we, R, S, P, loss, wo, N), "sn_loss_interlevel_forward")
def lb(t=F, w=F, te=F, we=F, g=F, R=4, S=8, P=16, ge=F):
    return done(lib.sn_loss_interlevel_backward(t, w, te, we, g, R, S, P, ge, N), "sn_loss_interlevel_backward")
calls = {
 "abi": lambda: "%d:text" % lib.sn_losses_abi_version(),
 "cf_S_0": lambda: cf(S=0), "cf_S_1025": lambda: cf(S=1025), "cf_R_neg": lambda: cf(R=-1), "cf_no_deltas": lambda: cf(deltas=N),
 "cf_no_density": lambda: cf(density=N), "cf_no_output": lambda: cf(w=N, rgb=N, acc=N), "cf_rgb_without_colour": lambda: cf(colour=N),
 "cb_S_0": lambda: cb(S=0), "cb_S_1025": lambda: cb(S=1025), "cb_R_neg": lambda: cb(R=-1), "cb_no_deltas": lambda: cb(deltas=N),
 "cb_no_density": lambda: cb(density=N), "cb_no_grad_density": lambda: cb(gd=N), "cb_grad_rgb_without_colour": lambda: cb(colour=N, gc=N),
 "cb_grad_colour_without_colour": lambda: cb(colour=N, grgb=N),
 "df_S_0": lambda: df(S=0), "df_S_1025": lambda: df(S=1025), "df_R_neg": lambda: df(R=-1), "df_no_t": lambda: df(t=N),
 "df_no_w": lambda: df(w=N), "df_no_loss": lambda: df(loss=N),
 "db_S_0": lambda: db(S=0), "db_S_1025": lambda: db(S=1025), "db_R_neg": lambda: db(R=-1), "db_no_t": lambda: db(t=N),
 "db_no_w": lambda: db(w=N), "db_no_g": lambda: db(g=N), "db_no_grad_w": lambda: db(gw=N),
 "lf_S_0": lambda: lf(S=0), "lf_S_1025": lambda: lf(S=1025), "lf_P_0": lambda: lf(P=0), "lf_P_1025": lambda: lf(P=1025),
 "lf_R_neg": lambda: lf(R=-1), "lf_no_t": lambda: lf(t=N), "lf_no_w": lambda: lf(w=N), "lf_no_t_env": lambda: lf(te=N),
 "lf_no_w_env": lambda: lf(we=N), "lf_no_output": lambda: lf(loss=N), "lf_loss_without_w": lambda: lf(w=N, wo=F),
 "lb_S_0": lambda: lb(S=0), "lb_S_1025": lambda: lb(S=1025), "lb_P_0": lambda: lb(P=0), "lb_P_1025": lambda: lb(P=1025),
 "lb_R_neg": lambda: lb(R=-1), "lb_no_t": lambda: lb(t=N), "lb_no_w": lambda: lb(w=N), "lb_no_t_env": lambda: lb(te=N),
 "lb_no_w_env": lambda: lb(we=N), "lb_no_g": lambda: lb(g=N), "lb_no_grad": lambda: lb(ge=N),
 "ok_cf_R_0": lambda: cf(R=0), "ok_cb_R_0": lambda: cb(R=0), "ok_df_R_0": lambda: df(R=0), "ok_db_R_0": lambda: db(R=0),
 "ok_lf_R_0": lambda: lf(R=0), "ok_lb_R_0": lambda: lb(R=0), "ok_cf_R_0_null": lambda: cf(R=0, deltas=N, density=N, colour=N, w=N, rgb=N, acc=N),
}
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_loss_entry_points_refuse_bad_arguments_before_the_device(built_lib):
    """S or P outside [1, 1024], a negative R, a NULL required pointer: SN_ERR_INVALID with the entry point's name in sn_last_error; R = 0 is
    SN_OK without a launch.  In a child process -- a crash would be a segfault -- and host-only: it runs without a GPU."""
    got = refusal_sweep(_SWEEP)
    want = {k: ("0:text" if k.startswith("ok_") else "1:text") for k in got}
    assert len(got) == 58 and got == want


def test_python_surface_refuses_before_the_device():
    from signerf_amd import losses

    x = torch.zeros(2, 4, 1)
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        losses.get_weights(x, x)
    with pytest.raises(TypeError, match="fp32"):
        losses.get_weights(x.double(), x.double())
    with pytest.raises(TypeError, match="fp32"):
        losses.lossfun_distortion(torch.zeros(2, 5, dtype=torch.float16), torch.zeros(2, 4, dtype=torch.float16))
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        losses.lossfun_outer(torch.zeros(2, 5), torch.zeros(2, 4), torch.zeros(2, 9), torch.zeros(2, 8))
    with pytest.raises(TypeError, match="Tensor"):
        losses.get_weights([1.0], x)
