"""Trainable MLP, CPU side: the restatement tests/mlp_oracle.py against ``oracle.nerfacto.mlp_forward`` and its formula gradients against
``torch.autograd`` in fp64, the validity of the exact-integer cases tests/test_gpu_mlp.py runs, the companion C header
include/signerf_hip_mlp.h against the binding, the library's exports and its argument refusals (in a child process: nothing is launched),
the workspace size against what the Python side allocates, and the Python surface that needs no device.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import mlp_oracle as mo
from abi_helpers import c99_probe, refusal_sweep
from helpers import onf, small_config
from signerf_amd import _lib, mlp
from signerf_amd.nerfacto import MLP

D = torch.float64
INTEGER_SIZES = [17, 130, 1000]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_restatement_in_fp32_is_the_oracles_forward():
    torch.manual_seed(0)
    net = MLP(10, 3, 16, 4)
    x = torch.randn(33, 10)
    params = {"m." + k: v.detach() for k, v in net.state_dict().items()}
    y, hs = mo.forward(x, [l.weight.detach() for l in net.layers], [l.bias.detach() for l in net.layers], torch.float32)
    assert torch.equal(y, onf.mlp_forward(x, params, "m", 3)) and len(hs) == 3 and torch.equal(hs[0], x)


@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_gradient_formulas_equal_autograd(dims):
    w, b = mo.linear_init(dims, seed=len(dims))
    x, g = mo.inputs(dims, 257, seed=3, kind="uniform")
    y, hs = mo.forward(x, w, b, D)
    want_y, want_x, want_w, want_b = mo.autograd(x, w, b, g, D)
    got_x, got_w, got_b = mo.backward(x, w, b, g, D)
    for got, want in [(y, want_y), (got_x, want_x)] + list(zip(got_w, want_w)) + list(zip(got_b, want_b)):
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300)


def test_the_relu_mask_is_torch_autograds_on_every_class_of_value():
    """z = NaN, +-inf, +-0 and finite values through relu: the formula's mask (h <= 0 blocks) is what autograd applies."""
    z = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 1.5, -1.5], dtype=D, requires_grad=True)
    h = torch.relu(z)
    h.backward(torch.full_like(z, 3.0))
    assert torch.equal(z.grad, torch.where(h.detach() <= 0, 0.0, 3.0).to(D)) and z.grad.tolist() == [3.0, 3.0, 0.0, 0.0, 0.0, 3.0, 0.0]


@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_integer_cases_are_exact_in_fp32_in_any_order(dims):
    """sum |terms| < 2^24 for every sum of the five outputs (an assertion, not a skip), at every N the GPU test uses and at the sizes the
    fp32 and fp64 restatements were compared at; and those two agree exactly."""
    for N in sorted(set(mo.SIZES + mo.LARGE_SIZES + INTEGER_SIZES)):
        x, w, b, g = mo.integer_case(dims, N)
        mo.assert_integer_case_is_valid(x, w, b, g)
        for t in [x, g] + w + b:
            assert torch.equal(t, t.round())
        assert all(0.3 < float((wi == 0).float().mean()) < 0.9 for wi in w if wi.numel() >= 256)
        if N in INTEGER_SIZES:
            y32, _ = mo.forward(x, w, b, torch.float32)
            y64, _ = mo.forward(x, w, b, D)
            assert torch.equal(y32.double(), y64)
            for a32, a64 in zip(_flat(mo.backward(x, w, b, g, torch.float32)), _flat(mo.backward(x, w, b, g, D))):
                assert torch.equal(a32.double(), a64)


def _flat(r):
    return [r[0]] + list(r[1]) + list(r[2])


# ---- the companion C header ------------------------------------------------------------------------------------------------------------
NAMES = ["sn_mlp_abi_version", "sn_mlp_backward", "sn_mlp_backward_workspace_bytes", "sn_mlp_forward"]
KERNELS = ["sn_train_mlp_forward_kernel", "sn_train_mlp_backward_kernel", "sn_train_mlp_reduce_kernel"]


def test_mlp_header_binding_and_exports_agree(built_lib):
    """(The header against the binding, the exports and build.HEADERS: tests/test_cabi.py, for every header.)"""
    assert sorted(_lib.header("mlp").functions) == NAMES
    lib = _lib.load()
    assert lib.sn_mlp_abi_version() == _lib.header("mlp").version == 1
    blob = open(built_lib, "rb").read()
    for k in KERNELS:
        assert 24 <= len(k) <= 99       # (names behind _Z23...: DESIGN.md §4 "Wide fields", "Kernel names")
        assert ("_Z%d%s11SnMlpParams" % (len(k), k)).encode() in blob
    assert (mlp.MAX_LAYERS, mlp.MAX_DIM) == (4, 64)


def test_mlp_header_compiles_as_c99_and_the_descriptor_has_the_bindings_layout(tmp_path):
    got = c99_probe(tmp_path, "signerf_hip_mlp.h", "%d %d %d %d %d %d %d",
                    "SN_MLP_ABI_VERSION, SN_MLP_MAX_LAYERS, SN_MLP_MAX_DIM, (int)sizeof(SnMlpDesc), (int)offsetof(SnMlpDesc, weights), "
                    "(int)offsetof(SnMlpDesc, grad_weights), (int)offsetof(SnMlpDesc, grad_biases)")
    S = _lib.SnMlpDesc
    assert got == [str(v) for v in (1, 4, 64, C.sizeof(S), S.weights.offset, S.grad_weights.offset, S.grad_biases.offset)]
    assert _lib.SnMlpDesc().struct_size == C.sizeof(S) == 160


_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
P = 0x1000   # never dereferenced: every call below is refused (or N == 0) before the device is touched
def done(st, name):
    msg = lib.sn_last_error(None)
    return "%d:%s" % (st, "text" if (st == 0 or (msg and name.encode() in msg)) else "notext")
def desc(dims=(63, 64, 64, 3), n_layers=None, size=None, w=P, b=P, gw=P, gb=P, holes=()):
    d = _lib.SnMlpDesc()
    d.n_layers = len(dims) - 1 if n_layers is None else n_layers
    for i, v in enumerate(dims[:5]):
        d.dims[i] = v
    for i in range(min(max(d.n_layers, 0), 4)):
        d.weights[i], d.biases[i], d.grad_weights[i], d.grad_biases[i] = w, b, gw, gb
    for name, i in holes:
        getattr(d, name)[i] = None
    if size is not None:
        d.struct_size = size
    return d
def fw(d="default", x=P, n=4, y=P, **kw):
    d = desc(**kw) if d == "default" else d
    return done(lib.sn_mlp_forward(C.byref(d) if d is not None else None, x, n, y, N), "sn_mlp_forward")
def bw(d="default", x=P, g=P, n=4, gx=P, ws=P, ws_bytes=1 << 30, **kw):
    d = desc(**kw) if d == "default" else d
    return done(lib.sn_mlp_backward(C.byref(d) if d is not None else None, x, g, n, gx, ws, ws_bytes, N), "sn_mlp_backward")
calls = {"abi": lambda: "%d:text" % lib.sn_mlp_abi_version()}
for tag, f in (("fw", fw), ("bw", bw)):
    calls.update({
     tag + "_N_neg": lambda f=f: f(n=-1), tag + "_N_2p31": lambda f=f: f(n=2**31), tag + "_no_desc": lambda f=f: f(d=None),
     tag + "_layers_0": lambda f=f: f(n_layers=0), tag + "_layers_5": lambda f=f: f(dims=(8, 8, 8, 8, 8), n_layers=5),
     tag + "_layers_neg": lambda f=f: f(n_layers=-1), tag + "_dim_0": lambda f=f: f(dims=(10, 0, 1)), tag + "_dim_65": lambda f=f: f(dims=(10, 65, 1)),
     tag + "_in_0": lambda f=f: f(dims=(0, 16, 1)), tag + "_in_65": lambda f=f: f(dims=(65, 16, 1)), tag + "_out_128": lambda f=f: f(dims=(32, 64, 128)),
     tag + "_dim_neg": lambda f=f: f(dims=(10, -16, 1)), tag + "_size_0": lambda f=f: f(size=0), tag + "_size_short": lambda f=f: f(size=96),
     tag + "_size_long": lambda f=f: f(size=168), tag + "_N_0_bad_dim": lambda f=f: f(n=0, dims=(10, 65, 1)),
     tag + "_no_x": lambda f=f: f(x=N), tag + "_no_weight": lambda f=f: f(holes=(("weights", 1),)), tag + "_no_bias": lambda f=f: f(holes=(("biases", 2),)),
     tag + "_x_misaligned": lambda f=f: f(x=P + 2), tag + "_weight_misaligned": lambda f=f: f(w=P + 1),
     "ok_" + tag + "_N_0": lambda f=f: f(n=0), "ok_" + tag + "_N_0_largest": lambda f=f: f(n=0, dims=(64, 64, 64, 64, 64)),
    })
need = lib.sn_mlp_backward_workspace_bytes(C.byref(desc()), 4)
calls.update({
 "fw_no_y": lambda: fw(y=N), "ok_fw_N_0_null": lambda: fw(n=0, x=N, y=N, w=N, b=N),
 "bw_no_grad_y": lambda: bw(g=N), "bw_no_output": lambda: bw(gx=N, gw=N, gb=N), "bw_half_a_group": lambda: bw(holes=(("grad_weights", 0),)),
 "bw_biases_without_weights": lambda: bw(gw=N), "bw_no_workspace": lambda: bw(ws=N), "bw_workspace_short": lambda: bw(ws_bytes=need - 1),
 "bw_grad_misaligned": lambda: bw(gb=P + 2), "bw_workspace_misaligned": lambda: bw(ws=P + 2),
 "ok_bw_N_0_null": lambda: bw(n=0, x=N, g=N, gx=N, ws=N, ws_bytes=0, w=N, b=N, gw=N, gb=N),
 "ws_no_desc": lambda: "%d:text" % (1 if lib.sn_mlp_backward_workspace_bytes(None, 4) == 0 else 0),
 "ws_bad_dim": lambda: "%d:text" % (1 if lib.sn_mlp_backward_workspace_bytes(C.byref(desc(dims=(10, 65, 1))), 4) == 0 else 0),
 "ws_bad_size": lambda: "%d:text" % (1 if lib.sn_mlp_backward_workspace_bytes(C.byref(desc(size=96)), 4) == 0 else 0),
 "ws_N_neg": lambda: "%d:text" % (1 if lib.sn_mlp_backward_workspace_bytes(C.byref(desc()), -1) == 0 else 0),
 "ws_N_2p31": lambda: "%d:text" % (1 if lib.sn_mlp_backward_workspace_bytes(C.byref(desc()), 2**31) == 0 else 0),
})
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_mlp_entry_points_refuse_bad_arguments_before_the_device(built_lib):
    """N < 0, N >= 2^31, a layer count or a width out of range, an unknown struct_size, a NULL required pointer, half a gradient group, a
    short or missing workspace, a misaligned pointer: SN_ERR_INVALID with the entry point's name in sn_last_error (the workspace query
    answers 0); N = 0 is SN_OK without a launch.  In a child process -- a crash would be a segfault -- and host-only."""
    got = refusal_sweep(_SWEEP)
    want = {k: ("0:text" if k.startswith("ok_") else "1:text") for k in got}
    assert len(got) == 1 + 2 * 23 + 16 and got == want


@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_workspace_bytes_are_monotone_in_N_and_what_python_allocates(built_lib, dims):
    lib = _lib.load()
    d = _lib.SnMlpDesc()
    d.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = v
    image = sum(dims[i + 1] * dims[i] + dims[i + 1] for i in range(len(dims) - 1))
    last = 0
    for N in list(range(1, 200)) + [1000, 16383, 16384, 16385, 196608, 1048576, 2**31 - 1]:
        got = lib.sn_mlp_backward_workspace_bytes(C.byref(d), N)
        assert got == 4 * mlp.workspace_floats(dims, N) == 4 * image * min((N + 63) // 64, 256) and got >= last > -1
        last = got
    assert last == 4 * image * 256


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses_before_the_device():
    x, w, b = torch.zeros(4, 10), [torch.zeros(16, 10), torch.zeros(1, 16)], [torch.zeros(16), torch.zeros(1)]
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        mlp.fused_mlp(x, w, b)
    with pytest.raises(TypeError, match="fp32"):
        mlp.fused_mlp(x.double(), w, b)
    with pytest.raises(TypeError, match="fp32"):
        mlp.fused_mlp(x, [w[0].half(), w[1]], b)
    with pytest.raises(TypeError, match="Tensor"):
        mlp.fused_mlp([[0.0] * 10], w, b)
    with pytest.raises(ValueError, match="as many"):
        mlp.fused_mlp(x, w, b[:1])
    for dims in [(10, 65, 1), (10,), (8, 8, 8, 8, 8, 8), (0, 4)]:
        with pytest.raises(ValueError, match="1..4 layers"):
            mlp.check_dims(dims)
    for dims in mo.STACKS:
        mlp.check_dims(dims)


def test_the_module_switch_keeps_state_dict_and_defaults():
    a, b = MLP(10, 3, 16, 4), MLP(10, 3, 16, 4, implementation="hip")
    assert a.implementation == "torch" and list(a.state_dict()) == list(b.state_dict()) and [n for n, _ in b.named_buffers()] == []
    x = torch.randn(5, 10)
    with pytest.raises(_lib.SignerfHipError, match="GPU"):      # a CPU tensor reaches the op and is refused there: there is no CPU path
        b(x)
    b.implementation = "torch"
    b.load_state_dict(a.state_dict())
    assert torch.equal(a(x), b(x))
    b.implementation = "cuda"
    with pytest.raises(ValueError, match="implementation"):
        b(x)


def test_training_mlp_config():
    assert small_config().training_mlp == "torch"
    with pytest.raises(ValueError, match="training_mlp"):
        small_config(training_mlp="bogus").setup()
    torch_model, hip_model = small_config().setup(), small_config(training_mlp="hip", predict_normals=True).setup()
    assert all(m.implementation == "torch" for m in torch_model.modules() if isinstance(m, MLP))
    stacks = [m for m in hip_model.modules() if isinstance(m, MLP)]
    assert len(stacks) == 5 and all(m.implementation == "hip" for m in stacks)
    assert [k for k in hip_model.state_dict()] == [k for k in small_config(predict_normals=True).setup().state_dict()]
    with pytest.raises(NotImplementedError, match="wide"):
        small_config(training_mlp="hip", hidden_dim=128, hidden_dim_color=128).setup()
    with pytest.raises(NotImplementedError, match="tiny-cuda-nn"):
        small_config(training_mlp="hip", implementation="tcnn").setup()


def test_a_module_without_the_attribute_runs_the_torch_ops():
    """What unpickling a whole MLP module saved before ``implementation`` existed gives: no instance attribute, the class default."""
    m = MLP(10, 2, 16, 1)
    x = torch.randn(5, 10)
    want = m(x)
    del m.__dict__["implementation"]
    assert m.implementation == "torch" and torch.equal(m(x), want)


# ---- resources -------------------------------------------------------------------------------------------------------------------------------
def test_the_mlp_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """csrc/sn_mlp.h compiled alone for the device with the library's code-generation flags: the resource remarks of the three kernels
    report no scratch, no spilled register of either kind and no dynamic stack.  (The backward kernel keeps its bounds checks inside the
    tile loop by a device the next compiler may see through -- DESIGN.md §4 "Trainable MLP", "Resources"; this is where that would show.)"""
    from signerf_amd import build

    (tmp_path / "tu.hip").write_text('#include <hip/hip_runtime.h>\n#include <cstdint>\n#include "sn_mlp.h"\n')
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
        u = usage["_Z%d%s11SnMlpParams" % (len(k), k)]
        print(k, u)
        assert (u["ScratchSize [bytes/lane]"], u["SGPRs Spill"], u["VGPRs Spill"], u["Dynamic Stack"]) == ("0", "0", "0", "False"), (k, u)
