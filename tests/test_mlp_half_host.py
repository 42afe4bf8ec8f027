"""Mixed-precision MLP, CPU side (SnMlpDesc.precision; csrc/sn_mlp_half.h): the descriptor field's refusals and defaults in a child process
(nothing is launched), the workspace size, the Python surface that needs no device, tests/mlp_half_oracle.py against itself -- the exact
integer cases and the fp32 restatement against the bounds tests/test_gpu_mlp_half.py gates the kernel with -- and the resource remarks of
the two new kernels compiled alone.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import mlp_half_oracle as ho
import mlp_oracle as mo
from abi_helpers import c99_probe, refusal_sweep
from helpers import small_config
from signerf_amd import _lib, mlp
from signerf_amd.nerfacto import MLP

D = torch.float64
KERNELS = ["sn_train_mlp_half_forward_kernel", "sn_train_mlp_half_backward_kernel"]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_precision_sits_in_the_slot_reserved_had(tmp_path):
    got = c99_probe(tmp_path, "signerf_hip_mlp.h", "%d %d %d %d %d",
                    "SN_MLP_PRECISION_FP32, SN_MLP_PRECISION_FP16, (int)offsetof(SnMlpDesc, precision), (int)sizeof(((SnMlpDesc*)0)->precision), "
                    "(int)sizeof(SnMlpDesc)")
    S = _lib.SnMlpDesc
    assert got == ["0", "1", "28", "4", "160"] == [str(v) for v in (mlp.PRECISIONS["fp32"], mlp.PRECISIONS["fp16"], S.precision.offset, S.precision.size, C.sizeof(S))]
    assert _lib.SnMlpDesc().precision == 0 and _lib.header("mlp").version == 1


_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
P = 0x1000   # never dereferenced: every call below is refused (or N == 0) before the device is touched
def done(st, name):
    msg = lib.sn_last_error(None)
    return "%d:%s" % (st, "text" if (st == 0 or (msg and name.encode() in msg and b"precision" in msg)) else "notext")
def desc(precision, dims=(63, 64, 64, 3)):
    d = _lib.SnMlpDesc()
    d.n_layers, d.precision = len(dims) - 1, precision
    for i, v in enumerate(dims):
        d.dims[i] = v
    for i in range(d.n_layers):
        d.weights[i], d.biases[i], d.grad_weights[i], d.grad_biases[i] = P, P, P, P
    return d
for precision in (2, -1, 0, 1, 255, -2**31):
    for n in (4, 0):
        tag = "%s_%d_N_%d" % ("ok" if precision in (0, 1) and n == 0 else "skip" if precision in (0, 1) else "bad", precision & 0xffffffff, n)
        if tag.startswith("skip"):      # (a valid descriptor with N > 0 would launch)
            continue
        d = desc(precision)
        print("fw_" + tag, done(lib.sn_mlp_forward(C.byref(d), P, n, P, None), "sn_mlp_forward"), flush=True)
        print("bw_" + tag, done(lib.sn_mlp_backward(C.byref(d), P, P, n, P, P, 1 << 30, None), "sn_mlp_backward"), flush=True)
    ws = lib.sn_mlp_backward_workspace_bytes(C.byref(desc(precision)), 1000)
    print("ws_%d" % (precision & 0xffffffff), "%d:text" % (1 if (ws == 0) == (precision not in (0, 1)) else 0), flush=True)
"""


def test_an_unknown_precision_is_refused_before_the_device(built_lib):
    """precision = 2, -1 (and 255, INT_MIN) are SN_ERR_INVALID from both entry points with the entry point's name in sn_last_error, at N > 0
    and at N = 0; the workspace query answers 0 for them and the usual size for 0 and 1; precision 0 and 1 with N = 0 are SN_OK."""
    got = refusal_sweep(_SWEEP)
    want = {k: ("1:text" if "bad" in k or k.startswith("ws_") else "0:text") for k in got}
    assert len(got) == 4 * 2 * 2 + 2 * 2 + 6 and got == want, got
    assert got["fw_ok_0_N_0"] == got["bw_ok_1_N_0"] == "0:text" and got["fw_bad_2_N_4"] == got["bw_bad_%d_N_4" % 0xffffffff] == "1:text"


@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_workspace_bytes_are_the_same_for_both_precisions(built_lib, dims):
    lib = _lib.load()
    for N in list(range(1, 200)) + [1000, 16383, 16384, 16385, 196608, 1048576, 2**31 - 1]:
        got = []
        for precision in (0, 1):
            d = _lib.SnMlpDesc()
            d.n_layers, d.precision = len(dims) - 1, precision
            for i, v in enumerate(dims):
                d.dims[i] = v
            got.append(lib.sn_mlp_backward_workspace_bytes(C.byref(d), N))
        assert got[0] == got[1] == 4 * mlp.workspace_floats(dims, N) > 0


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses_an_unknown_precision_before_the_device():
    x, w, b = torch.zeros(4, 10), [torch.zeros(16, 10), torch.zeros(1, 16)], [torch.zeros(16), torch.zeros(1)]
    for bad in ("fp64", "half", 1, None, "FP16"):
        with pytest.raises(ValueError, match="precision"):
            mlp.fused_mlp(x, w, b, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            mlp.mlp_forward(x, w, b, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            mlp.mlp_backward(x, w, b, torch.zeros(4, 1), precision=bad)
    # both known ones reach the device check, and the tensors stay fp32 under both: the TypeError texts hold
    for good in ("fp32", "fp16"):
        with pytest.raises(_lib.SignerfHipError, match="GPU"):
            mlp.fused_mlp(x, w, b, precision=good)
        with pytest.raises(TypeError, match="fp32"):
            mlp.fused_mlp(x.half(), w, b, precision=good)
        with pytest.raises(TypeError, match="fp32"):
            mlp.fused_mlp(x, [w[0].half(), w[1]], b, precision=good)
    assert mlp._desc([10, 16, 1], [], []).precision == 0 and mlp._desc([10, 16, 1], [], [], precision=mlp.check_precision("fp16")).precision == 1


def test_the_module_and_the_config_carry_the_precision():
    a = MLP(10, 3, 16, 4)
    assert a.precision == "fp32" and MLP.precision == "fp32"
    x = torch.randn(5, 10)
    want = a(x)
    a.precision = "fp16"
    with pytest.raises(ValueError, match='implementation="hip"'):        # the torch path is fp32 here
        a(x)
    a.implementation = "hip"
    with pytest.raises(_lib.SignerfHipError, match="GPU"):                # "fp16" reaches the op, which has no CPU path
        a(x)
    a.precision = "bf16"
    with pytest.raises(ValueError, match="precision"):
        a(x)
    del a.__dict__["precision"]
    a.implementation = "torch"
    assert torch.equal(a(x), want)
    # the model config
    assert small_config().training_mlp_precision == "fp32"
    with pytest.raises(NotImplementedError, match='training_mlp="hip"'):
        small_config(training_mlp_precision="fp16").setup()
    with pytest.raises(ValueError, match="precision"):
        small_config(training_mlp="hip", training_mlp_precision="fp8").setup()
    half = small_config(training_mlp="hip", training_mlp_precision="fp16", predict_normals=True).setup()
    full = small_config(training_mlp="hip", predict_normals=True).setup()
    plain = small_config(predict_normals=True).setup()
    stacks = [m for m in half.modules() if isinstance(m, MLP)]
    assert len(stacks) == 5 and all((m.implementation, m.precision) == ("hip", "fp16") for m in stacks)
    assert all((m.implementation, m.precision) == ("hip", "fp32") for m in full.modules() if isinstance(m, MLP))
    assert all((m.implementation, m.precision) == ("torch", "fp32") for m in plain.modules() if isinstance(m, MLP))
    assert list(half.state_dict()) == list(full.state_dict()) == list(plain.state_dict())
    assert [(n, p.shape, p.dtype) for n, p in half.named_parameters()] == [(n, p.shape, p.dtype) for n, p in plain.named_parameters()]


# ---- the oracle against itself -------------------------------------------------------------------------------------------------------------
def test_r16_is_ieee_fp16():
    t = torch.tensor([1.0, 1.0 + 2.0**-11, 1.0 + 3 * 2.0**-11, 65504.0, 65519.9, 65520.0, 1e30, -1e30, 2.0**-14, 2.0**-24, 2.0**-25, 1.0001 * 2.0**-25,
                      3e-8 * 0, float("nan"), float("inf")])
    got = ho.r16(t)
    want = [1.0, 1.0, 1.0 + 2.0**-9, 65504.0, 65504.0, float("inf"), float("inf"), -float("inf"), 2.0**-14, 2.0**-24, 0.0, 2.0**-24, 0.0]
    assert got[:13].tolist() == want and torch.isnan(got[13]) and got[14] == float("inf") and not ho.FLUSH_SUBNORMALS
    assert torch.equal(ho.r16(t.double())[:13], got[:13].double())
    # one rounding, not two: just above a midpoint an fp64 value goes up, though its fp32 neighbour IS the midpoint and would tie to even
    just_above = torch.tensor([1.0 + 2.0**-11 + 2.0**-30, 2.0**-25 + 2.0**-60, -(1.0 + 2.0**-11 + 2.0**-30)], dtype=D)
    assert ho.r16(just_above).tolist() == [1.0 + 2.0**-10, 2.0**-24, -(1.0 + 2.0**-10)]


@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_integer_cases_round_nowhere_and_are_exact_in_any_order(dims):
    """Every value that is rounded to fp16 is an integer of magnitude <= 2048 and every sum of |terms| stays below 2^24, at every size the
    GPU test uses (assertions, not skips); every matrix of 256 entries or more keeps at least 5 % non-zeros; the specification equals the
    plain fp64 network there (nothing rounds); and the fp32 restatement equals the fp64 specification bit for bit."""
    for N in sorted(set(ho.SIZES + [17, 130])):
        x, w, b, g = ho.integer_case(dims, N)
        top, terms = ho.integer_case_figures(x, w, b, g)
        assert top <= 2048 and terms < 2.0**24, (dims, N, top, terms)
        for t in [x, g] + w + b:
            assert torch.equal(t, t.round())
        assert all(float((wi != 0).float().mean()) >= 0.05 for wi in w if wi.numel() >= 256)
        spec = ho.outputs(x, w, b, g, D)
        plain = (mo.forward(x, w, b, D)[0],) + mo.backward(x, w, b, g, D)
        for (name, a), (_, r) in zip(ho.flat(spec), ho.flat(plain)):
            assert torch.equal(a, r), (dims, N, name)
        if N <= 1000:
            for seed in (None, 5):
                for (name, a), (_, r) in zip(ho.flat(ho.outputs(x, w, b, g, torch.float32, perm_seed=seed)), ho.flat(spec)):
                    assert a.dtype == torch.float32 and torch.equal(a.double(), r), (dims, N, name, seed)


@pytest.mark.parametrize("dims", mo.STACKS, ids=str)
def test_the_restatement_meets_the_gpu_gates_with_headroom(dims):
    """The fp32 restatement, its sums in a random order, at N = 4096 on the six random cases of the GPU test, held to the GPU test's gates
    with headroom: every element of every output within 0.5 x B_flip (the GPU gate: 1), and at most 3 % of the rows of y and of dx with an
    element above 1 x B_tight (the GPU gate: 5 % above 2 x B_tight, the 2 being the allowance for the matrix instruction's unspecified
    inner order).  Measured here over all stacks: at most 0.33 of B_flip, on the one-term stack (1, 1), whose two roundings fill two
    thirds of a bound of three; at most 2.0 % of the rows."""
    N = 4096
    for wscale in ho.WEIGHT_SCALES:
        for xscale in ho.INPUT_SCALES:
            x, w, b, g = ho.random_case(dims, N, wscale, xscale)
            spec, tight, flip, info = ho.bounds(x, w, b, g)
            got = ho.outputs(x, w, b, g, torch.float32, perm_seed=3)
            worst = max(float(((a.double() - s).abs() / f.clamp_min(1e-300)).max()) for (_, a), (_, s), (_, f) in zip(ho.flat(got), ho.flat(spec), ho.flat(flip)))
            rows = {k: ho.rows_above(got[j], spec[j], tight[k], 1.0) for j, k in enumerate(("y", "dx"))}
            print(f"[half oracle] {dims} w {wscale} x {xscale}: largest error / B_flip {worst:.3f}, rows above B_tight {rows} of {N} (cap {ho.row_cap(N)}), {info}")
            assert worst <= 0.5 and max(rows.values()) <= 0.03 * N < ho.row_cap(N), (dims, wscale, xscale, worst, rows)
            if xscale == 1e-4:
                assert info["subnormal_hidden"] > 0      # the case does ask the subnormal question


def test_the_bounds_see_a_wrong_rounding_point():
    """The row gate has teeth: an fp32 network (no rounding at all) puts more than the cap of rows of y and dx beyond 2 x B_tight on the
    same data.  (B_flip cannot tell: it allows every hidden value a whole fp16 step.)"""
    dims, N = (32, 64, 16), 1000
    x, w, b, g = ho.random_case(dims, N, None, 1.0)
    spec, tight, flip, _ = ho.bounds(x, w, b, g)
    y32 = mo.forward(x, w, b, torch.float32)[0]
    assert ho.rows_above(y32, spec[0], tight["y"], 2.0) > ho.row_cap(N)
    dx32 = mo.backward(x, w, b, g, torch.float32)[0]
    assert ho.rows_above(dx32, spec[1], tight["dx"], 2.0) > ho.row_cap(N)


# ---- resources -----------------------------------------------------------------------------------------------------------------------------
def test_the_half_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """csrc/sn_mlp_half.h compiled alone for the device with the library's code-generation flags (the method of tests/test_mlp_host.py): no
    scratch, no spilled register of either kind and no dynamic stack on the two new kernels; their names are longer than 23 characters
    (DESIGN.md §4 "Wide fields", "Kernel names")."""
    from signerf_amd import build

    (tmp_path / "tu.hip").write_text('#include <hip/hip_runtime.h>\n#include <cstdint>\n#include "sn_mlp_half.h"\n')
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
        assert len(k) > 23
        u = usage["_Z%d%s11SnMlpParams" % (len(k), k)]
        print(k, u)
        assert (u["ScratchSize [bytes/lane]"], u["SGPRs Spill"], u["VGPRs Spill"], u["Dynamic Stack"]) == ("0", "0", "0", "False"), (k, u)


def test_the_library_holds_the_half_kernels(built_lib):
    blob = open(built_lib, "rb").read()
    for k in KERNELS:
        assert ("_Z%d%s11SnMlpParams" % (len(k), k)).encode() in blob
