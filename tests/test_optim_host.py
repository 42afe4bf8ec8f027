"""The fused Adam step, CPU side: the host planner signerf_amd/csrc/sn_optim_plan.h as a stand-alone program (tests/c/optim_plan.cpp, plain
and under the address and undefined-behaviour sanitizers), the companion C header include/signerf_hip_optim.h against the binding and the
library's exports, the argument refusals of sn_adam_step (in a child process: nothing is launched), and the resource remarks of the three
kernels.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from abi_helpers import c99_probe, refusal_sweep
from helpers import ROOT
from signerf_amd import _lib

SRC = os.path.join(ROOT, "tests", "c", "optim_plan.cpp")
NAMES = ["sn_adam_step", "sn_adam_workspace_bytes", "sn_optim_abi_version"]
KERNELS = ["sn_optim_adam_stats_kernel", "sn_optim_adam_prologue_kernel", "sn_optim_adam_update_kernel"]


# ---- the planner ---------------------------------------------------------------------------------------------------------------------------
def _build(tmp, name, flags):
    exe = os.path.join(tmp, name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe], capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path, r = _build(str(tmp_path_factory.mktemp("optim_plan")), "optim_plan", [])
    assert r.returncode == 0, r.stderr[-3000:]
    return path


def _counts(stdout):
    words = stdout.split()
    return dict(zip(words[0::2], map(int, words[1::2])))


def test_every_plan_covers_every_element_once_and_no_chunk_crosses_a_tensor(exe):
    """Sizes 0, 1, 3, 4, 5, 255, 256, 257, 65539 in every rotation, 1 to 71 tensors (one launch takes 32), one to three groups that clip or
    do not, and tensors of more chunks than a grid has workgroups: the program counts what it checked."""
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    n = _counts(r.stdout)
    assert n["cases"] > 700 and n["batches"] > n["cases"] and n["chunks"] > 50_000 and n["partials"] > 10_000 and n["strided"] >= 4
    assert _lib.SN_ADAM_MAX_TENSORS == 32


def test_the_plan_under_address_and_undefined_behaviour_sanitizers(exe, tmp_path):
    san, r = _build(str(tmp_path), "optim_plan_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0 and any(w in r.stderr for w in ("libasan", "libubsan", "-lasan", "-lubsan", "fsanitize")):
        pytest.skip("this toolchain has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-3000:]
    plain = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=120)
    checked = subprocess.run([san, "check"], capture_output=True, text=True, timeout=300)
    assert checked.returncode == 0 and checked.stderr == "", checked.stderr[-3000:]
    assert checked.stdout == plain.stdout


@pytest.mark.parametrize("n_tensors,total", [(0, 0), (1, 1), (3, 10000), (9, 65539 + 1035), (71, 19_400_000), (1, 2**40)])
def test_workspace_size_is_the_headers_layout(built_lib, exe, n_tensors, total):
    lib = _lib.load()
    records, partials, size = map(int, subprocess.run([exe, "workspace", str(n_tensors), str(total)], capture_output=True, text=True, check=True).stdout.split())
    assert lib.sn_adam_workspace_bytes(n_tensors, total) == size == C.sizeof(_lib.SnAdamRecord) * n_tensors + 8 * (total // 4096 + n_tensors)
    assert (records, partials) == (0, C.sizeof(_lib.SnAdamRecord) * n_tensors)
    assert lib.sn_adam_workspace_bytes(-1, total) == 0 and lib.sn_adam_workspace_bytes(n_tensors, -1) == 0


# ---- the companion C header ------------------------------------------------------------------------------------------------------------
def test_optim_header_binding_and_exports_agree(built_lib):
    """(The header against the binding, the exports and build.HEADERS: tests/test_cabi.py, for every header.)"""
    assert sorted(_lib.header("optim").functions) == NAMES
    lib = _lib.load()
    assert lib.sn_optim_abi_version() == _lib.header("optim").version == 1
    blob = open(built_lib, "rb").read()
    for k in KERNELS:
        assert 24 <= len(k) <= 99       # (names behind _Z23...: DESIGN.md §4 "Wide fields", "Kernel names")
        assert ("_Z%d%s10SnAdamArgs" % (len(k), k)).encode() in blob


def test_optim_header_compiles_as_c99_and_the_structs_have_the_bindings_layout(tmp_path):
    fields = [("SnAdamTensor", f) for f in ("param", "grad", "exp_avg", "exp_avg_sq", "step", "n", "group")]
    fields += [("SnAdamGroup", f) for f in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_norm")]
    fields += [("SnAdamRecord", f) for f in ("skip", "grad_multiplier", "step_size", "sqrt_bc2", "grad_norm")]
    structs = ("SnAdamTensor", "SnAdamGroup", "SnAdamRecord")
    exprs = ["SN_OPTIM_ABI_VERSION", "SN_ADAM_MAX_TENSORS"] + ["(int)sizeof(%s)" % s for s in structs] + ["(int)offsetof(%s, %s)" % sf for sf in fields]
    got = c99_probe(tmp_path, "signerf_hip_optim.h", " ".join(["%d"] * len(exprs)), ", ".join(exprs))
    want = [1, 32] + [C.sizeof(getattr(_lib, s)) for s in structs] + [getattr(getattr(_lib, s), f).offset for s, f in fields]
    assert got == [str(v) for v in want]
    assert _lib.SnAdamTensor().struct_size == C.sizeof(_lib.SnAdamTensor) == 64 and _lib.SnAdamGroup().struct_size == 28
    assert C.sizeof(_lib.SnAdamRecord) == 24


_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
P = 0x1000   # never dereferenced: every call below is refused (or has nothing to do) before the device is touched
def done(st, name="sn_adam_step"):
    msg = lib.sn_last_error(None)
    return "%d:%s" % (st, "text" if (st == 0 or (msg and name.encode() in msg)) else "notext")
def tensors(count=2, sizes=None, **kw):
    T = (_lib.SnAdamTensor * count)()
    for i in range(count):
        T[i].struct_size = C.sizeof(_lib.SnAdamTensor)
        T[i].param, T[i].grad, T[i].exp_avg, T[i].exp_avg_sq, T[i].step, T[i].n, T[i].group = P, P, P, P, P, 5, i % 2
    at = kw.pop("at", count - 1)
    for k, v in kw.items():
        setattr(T[at], k, v)
    for i, s in (sizes or {}).items():
        T[i].struct_size = s
    return T
def groups(count=2, sizes=None, **kw):
    G = (_lib.SnAdamGroup * count)()
    for i in range(count):
        G[i].struct_size = C.sizeof(_lib.SnAdamGroup)
        G[i].lr, G[i].beta1, G[i].beta2, G[i].eps, G[i].weight_decay, G[i].max_norm = 1e-2, 0.9, 0.999, 1e-15, 0.0, float(i)
    at = kw.pop("at", count - 1)
    for k, v in kw.items():
        setattr(G[at], k, v)
    for i, s in (sizes or {}).items():
        G[i].struct_size = s
    return G
def step(T="default", nt=None, G="default", ng=None, scale=N, inf=N, ws=P, ws_bytes=1 << 30):
    T = tensors() if T == "default" else T
    G = groups() if G == "default" else G
    nt = (len(T) if T is not None else 2) if nt is None else nt
    ng = (len(G) if G is not None else 2) if ng is None else ng
    return done(lib.sn_adam_step(T, nt, G, ng, scale, inf, ws, ws_bytes, N))
need = lib.sn_adam_workspace_bytes(2, 10)
nan, S, SG = float("nan"), C.sizeof(_lib.SnAdamTensor), C.sizeof(_lib.SnAdamGroup)
calls = {
 "abi": lambda: "%d:text" % lib.sn_optim_abi_version(),
 "n_tensors_neg": lambda: step(nt=-1), "n_groups_neg": lambda: step(ng=-1), "n_groups_0": lambda: step(ng=0),
 "no_tensors": lambda: step(T=N), "no_groups": lambda: step(G=N),
 "tensor_size_0": lambda: step(T=tensors(sizes={0: 0})), "tensor_size_short": lambda: step(T=tensors(sizes={0: S - 8, 1: S - 8})),
 "tensor_size_long": lambda: step(T=tensors(sizes={0: S + 8, 1: S + 8})), "tensor_size_mixed": lambda: step(T=tensors(sizes={1: S - 8})),
 "group_size_0": lambda: step(G=groups(sizes={0: 0})), "group_size_long": lambda: step(G=groups(sizes={0: SG + 4, 1: SG + 4})),
 "group_size_mixed": lambda: step(G=groups(sizes={1: 0})),
 "n_neg": lambda: step(T=tensors(n=-1)), "n_neg_first": lambda: step(T=tensors(n=-5, at=0)), "group_neg": lambda: step(T=tensors(group=-1)),
 "group_high": lambda: step(T=tensors(group=2)), "group_high_empty_tensor": lambda: step(T=tensors(group=2, n=0)),
 "no_param": lambda: step(T=tensors(param=N)), "no_grad": lambda: step(T=tensors(grad=N)), "no_exp_avg": lambda: step(T=tensors(exp_avg=N)),
 "no_exp_avg_sq": lambda: step(T=tensors(exp_avg_sq=N)), "no_step": lambda: step(T=tensors(step=N)),
 "param_misaligned": lambda: step(T=tensors(param=P + 2)), "grad_misaligned": lambda: step(T=tensors(grad=P + 1)),
 "exp_avg_misaligned": lambda: step(T=tensors(exp_avg=P + 3)), "exp_avg_sq_misaligned": lambda: step(T=tensors(exp_avg_sq=P + 6)),
 "step_misaligned": lambda: step(T=tensors(step=P + 2)),
 "bad_tensor_behind_one_launch": lambda: step(T=tensors(count=40, n=-1)), "no_grad_behind_one_launch": lambda: step(T=tensors(count=70, grad=N, at=65)),
 "beta1_1": lambda: step(G=groups(beta1=1.0)), "beta1_neg": lambda: step(G=groups(beta1=-0.1)), "beta1_nan": lambda: step(G=groups(beta1=nan)),
 "beta2_1": lambda: step(G=groups(beta2=1.0, at=0)), "beta2_neg": lambda: step(G=groups(beta2=-1e-3)), "beta2_2": lambda: step(G=groups(beta2=2.0)),
 "eps_neg": lambda: step(G=groups(eps=-1e-8)), "eps_nan": lambda: step(G=groups(eps=nan)), "lr_nan": lambda: step(G=groups(lr=nan)),
 "max_norm_nan": lambda: step(G=groups(max_norm=nan)), "weight_decay_nan": lambda: step(G=groups(weight_decay=nan)),
 "unused_group_bad_beta": lambda: step(T=tensors(count=1), G=groups(beta1=1.5)),
 "no_workspace": lambda: step(ws=N), "workspace_short": lambda: step(ws_bytes=need - 1), "workspace_0": lambda: step(ws_bytes=0),
 "workspace_misaligned": lambda: step(ws=P + 4), "grad_scale_misaligned": lambda: step(scale=P + 2), "found_inf_misaligned": lambda: step(inf=P + 1),
 "ws_n_neg": lambda: "%d:text" % (1 if lib.sn_adam_workspace_bytes(-1, 10) == 0 else 0),
 "ws_total_neg": lambda: "%d:text" % (1 if lib.sn_adam_workspace_bytes(2, -1) == 0 else 0),
 "ok_n_tensors_0": lambda: step(nt=0), "ok_n_tensors_0_null": lambda: step(T=N, nt=0, G=N, ng=0, ws=N, ws_bytes=0),
 "ok_all_empty_null": lambda: step(T=tensors(count=1, n=0, param=N, grad=N, exp_avg=N, exp_avg_sq=N, step=N), ws=N, ws_bytes=0),
 "ok_all_empty_misaligned": lambda: step(T=tensors(count=1, n=0, param=P + 1, grad=P + 2)),
}
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_adam_step_refuses_bad_arguments_before_the_device(built_lib):
    """A negative count, a NULL array or required pointer, n < 0, a group outside the array, a pointer off 4 bytes, a beta outside [0, 1),
    eps < 0, a NaN hyper-parameter, an unknown struct_size, a missing, short or misaligned workspace: SN_ERR_INVALID with the entry point's
    name in sn_last_error; no tensors and only empty tensors are SN_OK without a launch and without a look at the pointers.  In a child
    process -- a crash would be a segfault -- and host-only."""
    got = refusal_sweep(_SWEEP)
    want = {k: ("0:text" if k.startswith("ok_") else "1:text") for k in got}
    assert len(got) == 54 and got == want


# ---- resources -------------------------------------------------------------------------------------------------------------------------------
def test_the_adam_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """csrc/sn_optim.h compiled alone for the device with the library's code-generation flags: the descriptors are indexed in the kernel
    arguments, which must not turn into a private copy."""
    from signerf_amd import build

    (tmp_path / "tu.hip").write_text('#include <hip/hip_runtime.h>\n#include <cstdint>\n#include "signerf_hip_optim.h"\n#include "sn_optim.h"\n')
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), f"--offload-arch={build.ARCH}", *build.CODEGEN_FLAGS, "--cuda-device-only", "-c",
                        "-I", build.CSRC, "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", str(tmp_path / "tu.hip"),
                        "-o", str(tmp_path / "tu.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for m in re.finditer(r"remark: +(.*?) +\[-Rpass-analysis", r.stderr):
        key, _, value = m.group(1).rpartition(":")
        if key == "Function Name":
            name = value.strip()
        elif name:
            usage.setdefault(name, {})[key.strip()] = value.strip()
    for k in KERNELS:
        u = usage["_Z%d%s10SnAdamArgs" % (len(k), k)]
        print(k, u)
        assert (u["ScratchSize [bytes/lane]"], u["SGPRs Spill"], u["VGPRs Spill"], u["Dynamic Stack"]) == ("0", "0", "0", "False"), (k, u)
