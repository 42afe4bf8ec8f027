"""Training-mode normals, CPU side: the restatement tests/train_normals_oracle.py against ``torch.autograd`` in fp64 and its committed seeds
against the caps the GPU tests rely on, the two companion C headers against the binding and the library's exports, the argument refusals
of the entry points (in a child process: nothing is launched), the order of the Python entry points' input checks, the config field, and
the kernels' resources.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import hashgrid_oracle as ho
import mlp_oracle as mo
import train_normals_oracle as to
from abi_helpers import c99_probe, refusal_sweep
from helpers import onf, small_config
from signerf_amd import _lib, train_normals

D = torch.float64
NAMES = {"train_normals": ["sn_train_normals_abi_version", "sn_train_normals_analytic"],
         "normal_losses": ["sn_loss_normals_backward", "sn_loss_normals_forward", "sn_normal_losses_abi_version"]}
KERNELS = ["_Z32sn_train_normals_analytic_kernelILi%dEEv20SnTrainNormalsParams" % f for f in (1, 2, 4, 8)] + \
          ["_Z30sn_loss_normals_forward_kernel19SnLossNormalsParams", "_Z31sn_loss_normals_backward_kernel19SnLossNormalsParams"]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [16, 5])
def test_the_formula_is_autograd_of_the_density_in_q(L):
    """g by formula = torch.autograd.grad of the stack's output channel 0 in the offsets, times the scales (fp64, fp32-decided cells) -- the
    way oracle.nerfacto.field_analytic_normals takes it -- and n = -F.normalize(g)."""
    (q, table, scalings, weights, biases), ref64, _ = to.references(L)
    idx, offset = ho.cells(q, scalings, to.LOG2_T)
    o = offset.to(D).clone().requires_grad_()
    h = ho.blend(ho.gather(table.to(D), idx), o).flatten(-2, -1)
    for i, (w, b) in enumerate(zip(weights, biases)):
        h = torch.nn.functional.linear(h, w.to(D), b.to(D))
        if i + 1 < len(weights):
            h = torch.relu(h)
    (g_o,) = torch.autograd.grad(h[:, 0].sum(), o)
    g = (g_o * scalings.to(D).view(1, -1, 1)).sum(1)
    assert float((g - ref64["g"]).abs().max()) <= 1e-12 * float(g.abs().max())
    assert float((-torch.nn.functional.normalize(g, dim=-1) - ref64["n"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("F", [1, 4, 8])
def test_the_feature_count_seeds_stay_under_the_caps(F):
    (q, table, scalings, weights, biases), ref64, ref32 = to.references(("F", F))
    L, stack = to.FEATURE_CASES[F]
    det = to.determined(ref64)
    assert int((~det).sum()) <= to.MAX_EXCLUDED * det.numel() and float(ref64["tie"].min()) >= to.TIE_REL
    assert table.shape == (L << to.LOG2_T, F) and stack[0] == L * F and tuple(weights[0].shape) == (stack[1], L * F)
    assert 0 < float((ref32["g"].double() - ref64["g"]).abs().max()) < 1e-3 * float(ref64["g"].abs().max())


@pytest.mark.parametrize("L", [16, 5])
def test_the_committed_seeds_stay_under_the_caps(L):
    """What the GPU tests rely on, from the fp64 reference alone: at most 2 % of the rows have no determined direction, no hidden unit sits
    on a ReLU tie (grad_q is compared on EVERY element), the special points are there, and the fp32 restatement's own error is non-zero."""
    (q, table, scalings, weights, biases), ref64, ref32 = to.references(L)
    det = to.determined(ref64)
    assert int((~det).sum()) <= to.MAX_EXCLUDED * det.numel()
    assert float(ref64["tie"].min()) >= to.TIE_REL
    assert q.shape == (to.N_POINTS, 3) and bool((q < 0).any()) and bool((q > 1).any()) and bool((q[1] == 0).all()) and q[0].tolist() == [0.25, 0.5, 0.75]
    assert table.shape == (L << to.LOG2_T, to.F) and scalings.shape == (L,) and tuple(weights[0].shape) == (to.STACKS[L][1], L * to.F)
    assert 0 < float((ref32["g"].double() - ref64["g"]).abs().max()) < 1e-3 * float(ref64["g"].abs().max())
    zero = to.analytic(*to.case(L, zero_row=True)[:3], to.LOG2_T, *to.case(L, zero_row=True)[3:], D)
    assert bool((zero["g"] == 0).all()) and bool((zero["n"] == 0).all())


def test_the_gate_can_fail():
    """A 1 % error of one level's scale (a coarse, a middle and the finest level) and a flipped sign exceed the limit."""
    (q, table, scalings, weights, biases), ref64, ref32 = to.references(16)
    det = to.determined(ref64)
    assert to.gate(ref32["g"], ref64["g"], ref32["g"])[0] and to.gate(ref32["n"], ref64["n"], ref32["n"], det)[0]
    for level in (0, 7, 15):
        s = scalings.clone().double()
        idx, offset = ho.cells(q, scalings, to.LOG2_T)
        s[level] *= 1.01
        f = ho.gather(table.to(D), idx)
        enc = ho.blend(f, offset.to(D)).flatten(-2, -1)
        one_hot = torch.zeros(q.shape[0], 16, dtype=D)
        one_hot[:, 0] = 1
        g = ho.grad_q_formula(f, offset, s, mo.backward(enc, weights, biases, one_hot, D)[0])
        assert not to.gate(g.float(), ref64["g"], ref32["g"])[0], level
    assert not to.gate(-ref32["n"], ref64["n"], ref32["n"], det)[0]


def test_loss_formulas_and_their_gradient():
    w, n, p, d = to.ray_inputs(7, 13, seed=1)
    o64, p64, rn64, rp64 = to.terms(w, n, p, d, D)
    assert o64.shape == p64.shape == (7,) and rn64.shape == rp64.shape == (7, 3) and bool((o64 >= 0).all())
    # by hand, sample by sample
    wd, nd, pd, dd = w.double(), n.double(), p.double(), d.double()
    for r in range(7):
        dots = [float(sum(nd[r, s, k] * -dd[r, k] for k in range(3))) for s in range(13)]
        assert float(o64[r]) == pytest.approx(sum(float(wd[r, s]) * min(0.0, dots[s]) ** 2 for s in range(13)), rel=1e-12, abs=1e-300)
        assert float(p64[r]) == pytest.approx(sum(float(wd[r, s]) * (1 - float((nd[r, s] * pd[r, s]).sum())) for s in range(13)), rel=1e-12)
    v = (wd[..., None] * nd).sum(1)
    assert torch.allclose(rn64, (v / (v.norm(dim=-1, keepdim=True) + 1e-10) + 1) / 2, rtol=0, atol=1e-15)
    assert torch.equal(rn64, onf.render_normals(nd, wd[..., None]))
    g = torch.linspace(-1, 2, 7, dtype=D)
    assert torch.allclose(to.pred_normal_grad(w, n, p, g, D), g[:, None, None] * wd[..., None] * -nd, rtol=0, atol=1e-15)
    # torch.fmin hands back the 0 where the dot product is NaN: the sample contributes w * 0
    n2 = n.clone()
    n2[0, 0, 0] = float("nan")
    assert bool(torch.isfinite(to.orientation_loss(wd, n2.double(), dd)).all())


# ---- the companion C headers ---------------------------------------------------------------------------------------------------------------
def test_headers_binding_and_exports_agree(built_lib):
    """(The headers against the binding, the exports and build.HEADERS: tests/test_cabi.py, for every header.)"""
    for key in NAMES:
        assert sorted(_lib.header(key).functions) == NAMES[key]
    lib = _lib.load()
    assert lib.sn_train_normals_abi_version() == _lib.header("train_normals").version == 1
    assert lib.sn_normal_losses_abi_version() == _lib.header("normal_losses").version == 1
    assert lib.sn_losses_abi_version() == 1 and lib.sn_mlp_abi_version() == 1 and lib.sn_hashgrid_abi_version() == 1     # (the siblings' stand)
    blob = open(built_lib, "rb").read()
    for k in KERNELS:
        assert k.encode() in blob, k
    build_headers = __import__("signerf_amd.build", fromlist=["x"]).HEADERS
    for h in ("sn_train_normals.h", "sn_normal_losses.h", "sn_api_train_normals.h", "sn_api_normal_losses.h"):
        assert h in build_headers


def test_headers_compile_as_c99(tmp_path):
    got = c99_probe(tmp_path, ("signerf_hip_train_normals.h", "signerf_hip_normal_losses.h"), "%d %d %d %d",
                    "SN_TRAIN_NORMALS_ABI_VERSION, SN_NORMAL_LOSSES_ABI_VERSION, SN_LOSSES_MAX_SAMPLES, SN_MLP_MAX_DIM")
    assert got == ["1", "1", "1024", "64"]


_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
P = 0x1000   # never dereferenced: every call below is refused (or N == 0 / R == 0) before the device is touched
def done(st, name):
    msg = lib.sn_last_error(None)
    return "%d:%s" % (st, "text" if (st == 0 or (msg and name.encode() in msg)) else "notext")
def desc(dims=(32, 64, 16), w=P, b=P, size=None):
    d = _lib.SnMlpDesc()
    d.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = v
    for i in range(d.n_layers):
        d.weights[i], d.biases[i] = w, b
    if size is not None:
        d.struct_size = size
    return d
def an(q=P, table=P, scal=P, n=4, L=16, log2_T=10, F=2, d="default", normals=P, grad=P, **kw):
    d = desc(**kw) if d == "default" else d
    return done(lib.sn_train_normals_analytic(q, table, scal, n, L, log2_T, F, C.byref(d) if d is not None else None, normals, grad, N),
                "sn_train_normals_analytic")
def fw(w=P, n=P, p=P, d=P, R=4, S=8, o=P, pn=P, rn=P, rp=P):
    return done(lib.sn_loss_normals_forward(w, n, p, d, R, S, o, pn, rn, rp, N), "sn_loss_normals_forward")
def bw(w=P, n=P, g=P, R=4, S=8, out=P):
    return done(lib.sn_loss_normals_backward(w, n, g, R, S, out, N), "sn_loss_normals_backward")
calls = {
 "an_N_neg": lambda: an(n=-1), "an_N_2p31": lambda: an(n=2**31), "an_no_desc": lambda: an(d=None), "an_desc_size": lambda: an(size=96),
 "an_dims0_small": lambda: an(dims=(10, 16, 1)), "an_dims0_at_L5": lambda: an(L=5), "an_dims0_at_F4": lambda: an(F=4), "an_dims0_N_0": lambda: an(n=0, L=5),
 "an_width_65": lambda: an(dims=(32, 65, 16)), "an_L_0": lambda: an(L=0, dims=(1, 1)), "an_L_33": lambda: an(L=33), "an_F_3": lambda: an(F=3),
 "an_log2_T_0": lambda: an(log2_T=0), "an_log2_T_25": lambda: an(log2_T=25), "an_no_q": lambda: an(q=N), "an_no_table": lambda: an(table=N),
 "an_no_scalings": lambda: an(scal=N), "an_no_normals": lambda: an(normals=N), "an_no_weight": lambda: an(w=N), "an_no_bias": lambda: an(b=N),
 "an_table_misaligned": lambda: an(table=P + 4), "an_q_misaligned": lambda: an(q=P + 2), "an_weight_misaligned": lambda: an(w=P + 1),
 "ok_an_N_0": lambda: an(n=0), "ok_an_N_0_null": lambda: an(n=0, q=N, table=N, scal=N, normals=N, grad=N, w=N, b=N),
 "ok_an_N_0_proposal": lambda: an(n=0, L=5, dims=(10, 16, 1)),
 "fw_R_neg": lambda: fw(R=-1), "fw_S_0": lambda: fw(S=0), "fw_S_1025": lambda: fw(S=1025), "fw_no_weights": lambda: fw(w=N), "fw_no_normals": lambda: fw(n=N),
 "fw_no_output": lambda: fw(o=N, pn=N, rn=N, rp=N), "fw_pred_without_pred_normals": lambda: fw(p=N, o=N, rn=N, rp=N),
 "fw_rendered_pred_without_pred_normals": lambda: fw(p=N, o=N, pn=N, rn=N), "fw_orientation_without_directions": lambda: fw(d=N),
 "ok_fw_R_0": lambda: fw(R=0, w=N, n=N, p=N, d=N, o=N, pn=N, rn=N, rp=N),
 "bw_R_neg": lambda: bw(R=-1), "bw_S_0": lambda: bw(S=0), "bw_S_1025": lambda: bw(S=1025), "bw_no_weights": lambda: bw(w=N), "bw_no_normals": lambda: bw(n=N),
 "bw_no_grad": lambda: bw(g=N), "bw_no_output": lambda: bw(out=N), "ok_bw_R_0": lambda: bw(R=0, w=N, n=N, g=N, out=N),
}
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_entry_points_refuse_bad_arguments_before_the_device(built_lib):
    """What signerf_hip_hashgrid.h, signerf_hip_mlp.h and signerf_hip_losses.h refuse, and dims[0] != L * F (also at N = 0): SN_ERR_INVALID
    with the entry point's name in sn_last_error; N = 0 / R = 0 is SN_OK without a launch.  In a child process, host-only."""
    got = refusal_sweep(_SWEEP)
    want = {k: ("0:text" if k.startswith("ok_") else "1:text") for k in got}
    assert len(got) == 26 + 10 + 8 and got == want


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------
def test_python_entry_points_check_dtype_then_device():
    """dtype (TypeError) before device (SignerfHipError: there is no CPU path) for the three entry points; the shape errors need GPU tensors
    and are tests/test_gpu_train_normals.py's and tests/test_gpu_normal_losses.py's."""
    (q, table, scalings, weights, biases), _, _ = to.references(5)
    args = (q, table, scalings, to.LOG2_T, weights, biases)
    for fn in (train_normals.analytic_normals, train_normals.analytic_normals_composed):
        with pytest.raises(_lib.SignerfHipError, match="GPU"):
            fn(*args)
        with pytest.raises(TypeError, match="fp32"):
            fn(q.double(), *args[1:])
        with pytest.raises(TypeError, match="fp32"):
            fn(q, table, scalings, to.LOG2_T, weights, [biases[0], biases[1].half()])      # (the last tensor: every dtype before any device)
        with pytest.raises(TypeError, match="Tensor"):
            fn(q.tolist(), *args[1:])
    w, n, p, d = to.ray_inputs(3, 5, seed=0)
    w = w[..., None]
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        train_normals.normal_losses(w, n, p, d)
    with pytest.raises(TypeError, match="fp32"):
        train_normals.normal_losses(w, n, p, d.double())
    with pytest.raises(TypeError, match="Tensor"):
        train_normals.normal_losses(w, n, None, d)
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        train_normals.render_normals(w, n)
    with pytest.raises(TypeError, match="fp32"):
        train_normals.render_normals(w, n.half())


def test_training_normals_config():
    from signerf_amd.config import NerfactoModelConfig

    assert NerfactoModelConfig().training_normals is False and small_config().training_normals is False
    assert small_config(training_normals=True).training_normals is True
    on, off = small_config(training_normals=True, predict_normals=True).setup(), small_config(predict_normals=True).setup()
    assert list(on.state_dict()) == list(off.state_dict())                    # a switch, not state


# ---- resources -------------------------------------------------------------------------------------------------------------------------------
def test_the_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """csrc/sn_train_normals.h and csrc/sn_normal_losses.h compiled alone for the device with the library's code-generation flags: the
    resource remarks report no scratch, no spilled register and no dynamic stack (the analytic kernel keeps the encoding, its slopes and
    the hidden activations of 16 points in registers)."""
    from signerf_amd import build

    inst = "".join("template __global__ void sn_train_normals_analytic_kernel<%d>(SnTrainNormalsParams);\n" % f for f in (1, 2, 4, 8))
    (tmp_path / "tu.hip").write_text('#include <hip/hip_runtime.h>\n#include <cstdint>\n#include "sn_train_normals.h"\n#include "sn_normal_losses.h"\n' + inst)
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), f"--offload-arch={build.ARCH}", *build.CODEGEN_FLAGS, "--cuda-device-only", "-c",
                        "-I", build.CSRC, "-Rpass-analysis=kernel-resource-usage", str(tmp_path / "tu.hip"), "-o", str(tmp_path / "tu.o")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for m in re.finditer(r"remark: +(.*?) +\[-Rpass-analysis", r.stderr):
        key, _, value = m.group(1).rpartition(":")
        if key == "Function Name":
            name = value.strip()
        elif name:
            usage.setdefault(name, {})[key.strip()] = value.strip()
    for k in KERNELS:
        u = usage[k]
        print(k, u)
        assert (u["ScratchSize [bytes/lane]"], u["SGPRs Spill"], u["VGPRs Spill"], u["Dynamic Stack"]) == ("0", "0", "0", "False"), (k, u)
    # sn_mlp.h's backward kernel, compiled in the same unit, keeps its two waves per SIMD, i.e. at most 256 registers of both kinds (it has
    # its own inline copy of the reverse step: sharing sn_mlp_layer_grad_in with it as a plain function cost 12 AGPRs and one of the waves)
    u = usage["_Z28sn_train_mlp_backward_kernel11SnMlpParams"]
    print("sn_train_mlp_backward_kernel", u)
    assert u["Occupancy [waves/SIMD]"] == "2" and int(u["VGPRs"]) + int(u["AGPRs"]) <= 256, u
