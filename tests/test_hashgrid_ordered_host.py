"""The ordered table gradient of the trainable hash grids, CPU side: the extension header signerf_amd/include/signerf_hip_hashgrid_ordered.h
against the binding, the library's exports and its argument refusals (in a child process: nothing is launched), the workspace query, the
Python surface and the config switch, and -- on the CPU, with plain torch sums -- that the gate the GPU tests apply,
|error| <= (2 + n 2^-29) 2^-24 A, separates an fp64 sum rounded once from an fp32 sum.  No GPU."""
import os

import pytest
import torch

import hashgrid_oracle as ho
from abi_helpers import c99_probe, declared, exported, refusal_sweep
from helpers import ROOT, small_config
from signerf_amd import _lib, hashgrid
from signerf_amd.nerfacto import HashEncoding

NAMES = ["sn_hashgrid_ordered_abi_version", "sn_hashgrid_ordered_backward", "sn_hashgrid_ordered_tcnn_backward", "sn_hashgrid_ordered_workspace_bytes"]
KERNELS = ["sn_hashgrid_ordered_emit_kernel", "sn_hashgrid_ordered_histogram_kernel", "sn_hashgrid_ordered_scan_digit_kernel",
           "sn_hashgrid_ordered_scatter_kernel", "sn_hashgrid_ordered_segment_sum_kernel"]
HEADER = os.path.join(_lib.EXTENSION_DIR, "signerf_hip_hashgrid_ordered.h")


def ordered_bound(n, A, calls=1):
    """The contract's bound per element: one fp32 rounding per product, an fp64 sum of n terms, one final fp32 rounding per call."""
    return (2.0 * calls + n.double() * 2.0**-29) * 2.0**-24 * A


# ---- the extension header ---------------------------------------------------------------------------------------------------------------
def test_header_binding_exports_version_and_build_agree(built_lib):
    from signerf_amd import build

    h = _lib.header("hashgrid_ordered")
    assert h in _lib.EXTENSIONS and h not in _lib.REGISTRY and not set(h.functions) & set(_lib.functions())
    assert h.file == os.path.basename(HEADER) and h.file not in os.listdir(os.path.join(ROOT, "include")) and not h.recorded
    assert declared(HEADER) == sorted(h.functions) == NAMES
    assert not sorted(set(h.functions) - exported(built_lib))
    assert h.version_fn in h.functions and h.version_macro == "SN_HASHGRID_ORDERED_ABI_VERSION"
    assert _lib.load().sn_hashgrid_ordered_abi_version() == h.version == 1
    assert os.path.join("..", "include", h.file) in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "..", "include", h.file))
    assert "sn_hashgrid_ordered.h" in build.HEADERS and "sn_api_hashgrid_ordered.h" in build.HEADERS
    lib = _lib.load()
    for name, (res, args) in h.functions.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    blob = open(built_lib, "rb").read()
    for k in KERNELS:
        assert len(k) > 23 and ("_Z%d%s" % (len(k), k)).encode() in blob, k     # DESIGN.md "Kernel names": behind _Z23sn_clip_expected_kernel
    for F in (1, 2, 4, 8):
        for grid in (b"13SnHgTorchGridE", b"12SnHgTcnnGridE"):
            assert b"_Z31sn_hashgrid_ordered_emit_kernelILi%dE" % F + grid in blob, (F, grid)
        assert b"_Z38sn_hashgrid_ordered_segment_sum_kernelILi%dEE" % F in blob, F


def test_header_compiles_as_c99(tmp_path):
    assert c99_probe(tmp_path, ("signerf_hip_hashgrid.h", HEADER), "%d %d", "SN_HASHGRID_ORDERED_ABI_VERSION, SN_HASHGRID_ORDERED_MAX_POINTS") == [
        "1", str(2**28 - 1)]


def test_the_siblings_are_what_they_were():
    """Opt-in: the two sibling headers keep their versions and their function lists."""
    assert _lib.header("hashgrid").version == 1 and sorted(_lib.header("hashgrid").functions) == [
        "sn_hashgrid_abi_version", "sn_hashgrid_backward", "sn_hashgrid_debug_reload_env", "sn_hashgrid_forward"]
    assert _lib.header("hashgrid_tcnn").version == 1 and len(_lib.header("hashgrid_tcnn").functions) == 4


# ---- the workspace ---------------------------------------------------------------------------------------------------------------------
def test_workspace_is_a_monotone_function_of_its_arguments(built_lib):
    ws = _lib.load().sn_hashgrid_ordered_workspace_bytes
    sizes = [ws(n, 16, 19, 2) for n in (1, 2, 63, 64, 65, 511, 512, 513, 4096, 196608, 1048576, 2**28 - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert sizes == [ws(n, 16, 19, 2) for n in (1, 2, 63, 64, 65, 511, 512, 513, 4096, 196608, 1048576, 2**28 - 1)]        # asked twice
    # at least the stored contributions, two (key, id) buffers and the counters of every tile; one level's worth, whatever L is
    for n, F in ((1, 1), (5000, 2), (196608, 2), (1048576, 8)):
        m = 8 * n
        assert ws(n, 5, 17, F) >= m * 4 * F + 4 * m * 4 + 257 * 4 * ((m + 4095) // 4096), (n, F)
        assert ws(n, 5, 17, F) == ws(n, 16, 17, F) == ws(n, 1, 17, F)
        assert ws(n, 5, 17, F) < 8 * n * (4 * F + 16) * 1.1 + 16384
    assert ws(196608, 16, 19, 2) < 2**26 and ws(1048576, 5, 17, 2) < 2**28          # the shapes of a step: 38 MB and 203 MB
    # 0 for N <= 0 and for every argument the entry points refuse
    for bad in ((0, 16, 19, 2), (-1, 16, 19, 2), (2**28, 16, 19, 2), (2**31, 16, 19, 2), (4, 0, 19, 2), (4, 33, 19, 2), (4, 16, 0, 2), (4, 16, 25, 2),
                (4, 16, 19, 0), (4, 16, 19, 3), (4, 16, 19, 16), (4, 32, 24, 4), (4, 16, 24, 8)):
        assert ws(*bad) == 0, bad


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
_SWEEP = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from signerf_amd import _lib
lib = _lib.load()
N = None
P = 0x1000   # never dereferenced: every call below is refused (or N == 0) before the device is touched
BIG = 1 << 40
def done(st, name, needle=b""):
    msg = lib.sn_last_error(None)
    return "%d:%s" % (st, "text" if (st == 0 or (msg and name.encode() in msg and needle in msg)) else "notext")
def make(name):
    fn = getattr(lib, name)
    def bw(q=P, table=P, s=P, g=P, n=4, L=16, T=19, F=2, gt=P, gq=P, ws=P, size=BIG, needle=b""):
        return done(fn(q, table, s, g, n, L, T, F, gt, gq, ws, size, N), name, needle)
    return bw
calls = {"abi": lambda: "%d:text" % lib.sn_hashgrid_ordered_abi_version()}
for tag, f in (("torch", make("sn_hashgrid_ordered_backward")), ("tcnn", make("sn_hashgrid_ordered_tcnn_backward"))):
    need = lib.sn_hashgrid_ordered_workspace_bytes(4, 16, 19, 2)
    calls.update({
     tag + "_N_neg": lambda f=f: f(n=-1), tag + "_N_2p31": lambda f=f: f(n=2**31), tag + "_N_2p28": lambda f=f: f(n=2**28, needle=b"2^28"),
     tag + "_N_2p30": lambda f=f: f(n=2**30, needle=b"2^28"),
     tag + "_L_0": lambda f=f: f(L=0), tag + "_L_33": lambda f=f: f(L=33),
     tag + "_T_0": lambda f=f: f(T=0), tag + "_T_25": lambda f=f: f(T=25), tag + "_F_0": lambda f=f: f(F=0), tag + "_F_3": lambda f=f: f(F=3),
     tag + "_F_16": lambda f=f: f(F=16), tag + "_F_neg": lambda f=f: f(F=-2), tag + "_table_2p31_a": lambda f=f: f(L=32, T=24, F=4),
     tag + "_table_2p31_b": lambda f=f: f(L=16, T=24, F=8), tag + "_table_2p31_c": lambda f=f: f(L=32, T=23, F=8),
     tag + "_N_0_bad_L": lambda f=f: f(n=0, L=0), tag + "_no_q": lambda f=f: f(q=N), tag + "_no_scalings": lambda f=f: f(s=N),
     tag + "_no_grad_enc": lambda f=f: f(g=N), tag + "_no_output": lambda f=f: f(gt=N, gq=N), tag + "_grad_q_without_table": lambda f=f: f(table=N, gt=N),
     tag + "_table_misaligned": lambda f=f: f(table=P + 4), tag + "_table_misaligned_F8": lambda f=f: f(table=P + 8, F=8),
     tag + "_grad_enc_misaligned": lambda f=f: f(g=P + 4), tag + "_grad_table_misaligned": lambda f=f: f(gt=P + 4),
     tag + "_no_workspace": lambda f=f: f(ws=N, needle=b"workspace"), tag + "_workspace_misaligned": lambda f=f: f(ws=P + 8, needle=b"workspace"),
     tag + "_workspace_small": lambda f=f, need=need: f(size=need - 1, needle=b"workspace"), tag + "_workspace_zero": lambda f=f: f(size=0, needle=b"workspace"),
     "ok_" + tag + "_N_0": lambda f=f: f(n=0), "ok_" + tag + "_N_0_largest_table": lambda f=f: f(n=0, L=32, T=24, F=2),
     "ok_" + tag + "_N_0_null": lambda f=f: f(n=0, q=N, table=N, s=N, g=N, gt=N, gq=N, ws=N, size=0),
    })
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_entry_points_refuse_bad_arguments_before_the_device(built_lib):
    """SN_ERR_INVALID with the entry point's OWN name (and, where the contract names a cause, that cause) in sn_last_error; N = 0 is SN_OK
    without a launch.  In a child process -- a crash would be a segfault -- and host-only.  (A grad_q-only call needs no workspace: that it
    then launches is the GPU tests' to show.)"""
    got = refusal_sweep(_SWEEP)
    want = {k: ("0:text" if k.startswith("ok_") else "1:text") for k in got}
    want["abi"] = "1:text"
    assert len(got) == 1 + 2 * 32 and got == want


# ---- the Python surface and the config switch -----------------------------------------------------------------------------------------
def test_python_surface_refuses_before_the_device():
    q, table, s = torch.zeros(4, 3), torch.zeros(5 << 4, 2), torch.tensor([16.0, 27.0, 45.0, 76.0, 128.0])
    for grid in ("torch", "tcnn"):
        with pytest.raises(ValueError, match="table_grad"):
            hashgrid.hash_encode(q, table, s, 4, grid=grid, table_grad="nope")
        with pytest.raises(ValueError, match="table_grad"):
            hashgrid.hash_encode_backward(q, table, s, 4, torch.zeros(4, 10), want_grad_q=True, grid=grid, table_grad="sorted")
        with pytest.raises(_lib.SignerfHipError, match="GPU"):
            hashgrid.hash_encode(q, table, s, 4, grid=grid, table_grad="ordered")
        with pytest.raises(_lib.SignerfHipError, match="GPU"):
            hashgrid.hash_encode_backward(q, table, s, 4, torch.zeros(4, 10), torch.zeros_like(table), grid=grid, table_grad="ordered")
        with pytest.raises(TypeError, match="fp32"):
            hashgrid.hash_encode(q.double(), table, s, 4, grid=grid, table_grad="ordered")
    assert hashgrid.TABLE_GRADS == ("atomic", "ordered") and set(hashgrid.ORDERED) == set(hashgrid.GRIDS)


def test_the_config_switch_reaches_every_grid_and_is_not_state():
    assert HashEncoding.table_grad == "atomic" and "table_grad" not in HashEncoding(5, 16, 128, 4).__dict__
    plain = small_config(training_forward=True).setup()
    assert plain.config.training_hashgrid_grad == "atomic"
    assert all(m.table_grad == "atomic" and "table_grad" not in m.__dict__ for m in plain.modules() if isinstance(m, HashEncoding))
    for kw in (dict(), dict(implementation="tcnn", training_tcnn=True)):
        model = small_config(training_forward=True, training_mlp="hip", training_hashgrid_grad="ordered", **kw).setup()
        grids = [m for m in model.modules() if isinstance(m, HashEncoding)]
        assert len(grids) == 3 and all(m.table_grad == "ordered" for m in grids)
        assert list(model.state_dict()) == list(small_config(training_forward=True, training_mlp="hip", **kw).setup().state_dict())
        with pytest.raises(_lib.SignerfHipError, match="GPU"):          # the op is reached, and has no CPU path
            grids[0](torch.rand(7, 3))
    with pytest.raises(ValueError, match="training_hashgrid_grad"):
        small_config(training_hashgrid_grad="sorted").setup()


# ---- the gate is worth something -------------------------------------------------------------------------------------------------------
def _collision_case(seed=0):
    """N = 5000 uniform points on ONE level of 16 rows (scaling 16, F = 2), grad_enc all positive: about 2500 contributions per element."""
    N, L, log2_T, F = 5000, 1, 4, 2
    q = ho.points(N, seed=seed, special=False)
    s = torch.tensor([16.0])
    g = torch.rand(N, L * F, generator=torch.Generator().manual_seed(seed + 1)) + 0.5
    idx, offset = ho.cells(q, s, log2_T)
    return q, s, g, idx, offset, L << log2_T, F


def test_an_fp64_sum_meets_the_bound_and_an_fp32_sum_does_not():
    """The contribution list of every element in contribution-id order (8 n + k), each product formed in fp64 and rounded to fp32 as the
    kernels do.  Summed in order in fp64 and rounded once it meets (2 + n 2^-29) 2^-24 A on every element; summed in order in fp32 (the
    best an fp32 sum can do without knowing the data: n - 1 roundings, expected error about sqrt(n / 3) 2^-25 A) it misses it.  Seed 0
    separates the two."""
    q, s, g, idx, offset, rows, F = _collision_case(seed=0)
    N = q.shape[0]
    w = ho.corner_weights(offset.double())                                  # [N,1,8]
    c32 = (w[..., None] * g.double().view(N, 1, 1, F)).to(torch.float32).reshape(N * 8, F)          # by contribution id
    row = idx.reshape(N * 8)
    ref, _ = ho.grads(q, torch.zeros(rows, F), s, 4, g, torch.float64)
    n, A = ho.contributions(idx, offset, g, rows)
    bound = ordered_bound(n, A)
    assert int(n.min()) > 2000 and int(n[:, 0].sum()) == 8 * N
    # every row's list in ascending contribution id, padded with zeros to the longest: one sequential sum per element, all rows at once
    # (an explicit loop of tensor adds: every fp32 add rounds to fp32, which torch's cumsum on the CPU, accumulating in fp64, would not)
    lists = torch.zeros(rows, int(n.max()), F)
    for r in range(rows):
        mine = c32[row == r]
        lists[r, :len(mine)] = mine
    in64, in32 = torch.zeros(rows, F, dtype=torch.float64), torch.zeros(rows, F, dtype=torch.float32)
    for j in range(lists.shape[1]):
        in64 += lists[:, j].double()
        in32 += lists[:, j]
    e64 = ((in64.to(torch.float32).double() - ref).abs() / bound).max()
    e32 = ((in32.double() - ref).abs() / bound).max()
    every32 = ((in32.double() - ref).abs() / bound)
    print(f"\n[ordered gate] n {int(n.min())}..{int(n.max())}; worst error / bound: fp64 sum rounded once {float(e64):.3f}, in-order fp32 sum {float(e32):.3f} "
          f"(median over the elements {float(every32.median()):.3f})")
    assert float(e64) <= 1.0
    assert float(e32) > 1.0
    # and the existing bound of the atomic form, (n + 4) 2^-24 A, is met by both: it could not tell them apart
    assert bool(((in32.double() - ref).abs() <= ho.grad_table_bound(n, A)).all())
