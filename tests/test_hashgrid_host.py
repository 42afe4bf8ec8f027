"""Trainable hash grid, CPU side: the restatement tests/hashgrid_oracle.py against ``oracle.nerfacto.hash_encode`` bit for bit, the
hand-derived gradient formulas (what csrc/sn_hashgrid.h implements) against ``torch.autograd`` in fp64, the wrapping uint32 hash against the
oracle's int64 one, the companion C header include/signerf_hip_hashgrid.h against the binding, the library's exports and its argument
refusals (in a child process: nothing is launched), and the Python surface that needs no device.  No GPU."""
import os

import numpy as np
import pytest
import torch

import hashgrid_oracle as ho
from abi_helpers import c99_probe, refusal_sweep
from helpers import ROOT, onf
from signerf_amd import _lib
from signerf_amd.nerfacto import MLP, HashEncoding, MLPWithHashEncoding

HEADER = os.path.join(ROOT, "include", "signerf_hip_hashgrid.h")
D = torch.float64
SHAPES = [(1, 1, 16, 16, 2), (5, 1, 16, 128, 2), (16, 4, 16, 2048, 1), (16, 10, 16, 2048, 2), (5, 17, 16, 128, 4), (3, 6, 16, 64, 8)]


def _case(L, log2_T, base, mx, F, N=257, lo=0.0, hi=1.0):
    return ho.points(N, seed=L + log2_T, lo=lo, hi=hi), ho.table(L, log2_T, F, seed=7), onf.hash_scalings(L, base, mx)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,log2_T,base,mx,F", SHAPES)
def test_restatement_in_fp32_is_the_oracle_bit_for_bit(L, log2_T, base, mx, F):
    for lo_, hi_ in ((0.0, 1.0), (-0.5, 1.5)):
        q, table, s = _case(L, log2_T, base, mx, F, lo=lo_, hi=hi_)
        enc, idx = ho.encode(q, table, s, log2_T, torch.float32)
        want = onf.hash_encode(q, table, s, log2_T)
        assert enc.shape == (q.shape[0], L * F) and torch.equal(enc.view(torch.int32), want.view(torch.int32))
        assert int(idx.min()) >= 0 and int(idx.max()) < L << log2_T
        assert torch.equal(idx // (1 << log2_T), torch.arange(L).view(1, L, 1).expand_as(idx))


def test_a_point_on_a_lattice_plane_has_both_corners_on_one_row():
    q = torch.tensor([[0.25, 0.3, 0.7]])
    idx, off = ho.cells(q, torch.tensor([16.0]), 10)
    assert float(off[0, 0, 0]) == 0.0
    # x: ceil == floor, so the corners that differ in x alone share their row (0 ccc / 3 fcc, 1 cfc / 2 ffc, 4 ccf / 7 fcf, 5 cff / 6 fff)
    for a, b in ((0, 3), (1, 2), (4, 7), (5, 6)):
        assert int(idx[0, 0, a]) == int(idx[0, 0, b])
    w = ho.corner_weights(off.double())
    assert [float(w[0, 0, k]) for k in (0, 1, 4, 5)] == [0.0] * 4 and float(w.sum()) == pytest.approx(1.0, abs=1e-15)


# ---- the hand-derived gradients against autograd, fp64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("L,log2_T,base,mx,F", SHAPES)
def test_gradient_formulas_equal_autograd(L, log2_T, base, mx, F):
    q, table, s = _case(L, log2_T, base, mx, F)
    g = torch.randn(q.shape[0], L * F, generator=torch.Generator().manual_seed(3), dtype=D)
    want_t, want_q = ho.grads(q, table, s, log2_T, g, D)
    idx, off = ho.cells(q, s, log2_T)
    got_t = ho.grad_table_formula(idx, off, g, table.shape[0])
    got_q = ho.grad_q_formula(ho.gather(table.to(D), idx), off, s, g)
    assert float((got_t - want_t).abs().max()) <= 1e-12 * float(want_t.abs().max())
    assert float((got_q - want_q).abs().max()) <= 1e-12 * float(want_q.abs().max())
    w = ho.corner_weights(off.double())
    assert float(w.min()) >= 0.0 and float(w.max()) <= 1.0 and float((w.sum(-1) - 1).abs().max()) <= 1e-14
    n, A = ho.contributions(idx, off, g, table.shape[0])
    assert int(n[:, 0].sum()) == q.shape[0] * L * 8 and bool((A >= 0).all()) and bool((A[n == 0] == 0).all())
    assert bool((got_t.abs() <= A * (1 + 1e-12)).all())


# ---- the hash ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2_T", [1, 4, 17, 19, 24])
def test_wrapping_uint32_hash_equals_the_int64_hash(log2_T):
    """What the kernels compute -- products in wrapping uint32, ``& (T - 1)`` -- against oracle.nerfacto.hash_fn (int64 products, ``%``),
    for random int32 coordinates, negative ones and the extremes included."""
    rng = np.random.default_rng(log2_T)
    L, T = 3, 1 << log2_T
    c = rng.integers(-2**31, 2**31, size=(5000, L, 3), dtype=np.int64).astype(np.int32)
    c[:8, 0] = [[0, 0, 0], [-1, -1, -1], [2**31 - 1] * 3, [-2**31] * 3, [-1, 0, 1], [1, -2**31, 2**31 - 1], [-2**30, 2**30, -1], [7, -7, 0]]
    want = onf.hash_fn(torch.from_numpy(c), T, torch.arange(L) * T).numpy()
    u = c.astype(np.uint32)
    with np.errstate(over="ignore"):
        h = (u[..., 0] * np.uint32(1)) ^ (u[..., 1] * np.uint32(2654435761)) ^ (u[..., 2] * np.uint32(805459861))
    got = (h & np.uint32(T - 1)).astype(np.int64) + np.arange(L, dtype=np.int64) * T
    assert np.array_equal(got, want)


# ---- the companion C header ------------------------------------------------------------------------------------------------------------
NAMES = ["sn_hashgrid_abi_version", "sn_hashgrid_backward", "sn_hashgrid_debug_reload_env", "sn_hashgrid_forward"]
KERNELS = ["sn_hashgrid_forward_kernel", "sn_hashgrid_backward_table_kernel", "sn_hashgrid_backward_input_kernel"]


def test_hashgrid_header_binding_and_exports_agree(built_lib):
    """(The header against the binding, the exports and build.HEADERS: tests/test_cabi.py, for every header.)"""
    assert sorted(_lib.header("hashgrid").functions) == NAMES
    lib = _lib.load()
    assert lib.sn_hashgrid_abi_version() == _lib.header("hashgrid").version == 1
    blob = open(built_lib, "rb").read()
    for k in KERNELS:
        assert 24 <= len(k) <= 99       # (names behind _Z23...: DESIGN.md §4 "Wide fields", "Kernel names")
        for F in (1, 2, 4, 8):
            assert ("_Z%d%sILi%dE" % (len(k), k, F)).encode() in blob


def test_hashgrid_header_compiles_as_c99(tmp_path):
    assert c99_probe(tmp_path, "signerf_hip_hashgrid.h", "%d %d %d",
                     "SN_HASHGRID_ABI_VERSION, SN_HASHGRID_MAX_LEVELS, SN_HASHGRID_MAX_LOG2_T") == ["1", "32", "24"]


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
def fw(q=P, table=P, s=P, n=4, L=16, T=19, F=2, enc=P, idx=N):
    return done(lib.sn_hashgrid_forward(q, table, s, n, L, T, F, enc, idx, N), "sn_hashgrid_forward")
def bw(q=P, table=P, s=P, g=P, n=4, L=16, T=19, F=2, gt=P, gq=P):
    return done(lib.sn_hashgrid_backward(q, table, s, g, n, L, T, F, gt, gq, N), "sn_hashgrid_backward")
calls = {"abi": lambda: "%d:text" % lib.sn_hashgrid_abi_version()}
for tag, f in (("fw", fw), ("bw", bw)):
    calls.update({
     tag + "_N_neg": lambda f=f: f(n=-1), tag + "_N_2p31": lambda f=f: f(n=2**31), tag + "_L_0": lambda f=f: f(L=0), tag + "_L_33": lambda f=f: f(L=33),
     tag + "_T_0": lambda f=f: f(T=0), tag + "_T_25": lambda f=f: f(T=25), tag + "_F_0": lambda f=f: f(F=0), tag + "_F_3": lambda f=f: f(F=3),
     tag + "_F_16": lambda f=f: f(F=16), tag + "_F_neg": lambda f=f: f(F=-2), tag + "_table_2p31_a": lambda f=f: f(L=32, T=24, F=4),
     tag + "_table_2p31_b": lambda f=f: f(L=16, T=24, F=8), tag + "_table_2p31_c": lambda f=f: f(L=32, T=23, F=8),
     tag + "_N_0_bad_L": lambda f=f: f(n=0, L=0), tag + "_no_q": lambda f=f: f(q=N), tag + "_no_scalings": lambda f=f: f(s=N),
     tag + "_table_misaligned": lambda f=f: f(table=P + 4), tag + "_table_misaligned_F8": lambda f=f: f(table=P + 8, F=8),
     "ok_" + tag + "_N_0": lambda f=f: f(n=0), "ok_" + tag + "_N_0_largest_table": lambda f=f: f(n=0, L=32, T=24, F=2),
    })
calls.update({
 "fw_no_table": lambda: fw(table=N), "fw_no_enc": lambda: fw(enc=N), "fw_enc_misaligned": lambda: fw(enc=P + 4), "fw_idx_misaligned": lambda: fw(idx=P + 8),
 "ok_fw_N_0_null": lambda: fw(n=0, q=N, table=N, s=N, enc=N),
 "bw_no_grad_enc": lambda: bw(g=N), "bw_no_output": lambda: bw(gt=N, gq=N), "bw_grad_q_without_table": lambda: bw(table=N, gt=N),
 "bw_grad_enc_misaligned": lambda: bw(g=P + 4), "bw_grad_table_misaligned": lambda: bw(gt=P + 4),
 "ok_bw_N_0_null": lambda: bw(n=0, q=N, table=N, s=N, g=N, gt=N, gq=N),
})
for k, f in calls.items():
    print(k, f(), flush=True)
"""


def test_hashgrid_entry_points_refuse_bad_arguments_before_the_device(built_lib):
    """A value outside its range, a table of 2^31 elements, a NULL required pointer, a misaligned row pointer: SN_ERR_INVALID with the entry
    point's name in sn_last_error; N = 0 is SN_OK without a launch.  In a child process -- a crash would be a segfault -- and host-only."""
    got = refusal_sweep(_SWEEP)
    want = {k: ("0:text" if k.startswith("ok_") else "1:text") for k in got}
    want["abi"] = "1:text"
    assert len(got) == 52 and got == want


# ---- the Python surface --------------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses_before_the_device():
    from signerf_amd import hashgrid

    q, table, s = torch.zeros(4, 3), torch.zeros(5 << 4, 2), onf.hash_scalings(5, 16, 128)
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        hashgrid.hash_encode(q, table, s, 4)
    with pytest.raises(TypeError, match="fp32"):
        hashgrid.hash_encode(q.double(), table, s, 4)
    with pytest.raises(TypeError, match="fp32"):
        hashgrid.hash_encode(q, table.half(), s, 4)
    with pytest.raises(TypeError, match="Tensor"):
        hashgrid.hash_encode([[0.0, 0.0, 0.0]], table, s, 4)


def test_modules_have_a_forward_and_keep_their_state_dict():
    """The state-dict key set is what it was before the modules had a forward: the scalings are a cached tensor, not a buffer."""
    enc = HashEncoding(5, 16, 128, 4)
    net = MLPWithHashEncoding(5, 16, 128, 4, 2, 2, 16, 1)
    keys = ["encoder.hash_table", "mlp.layers.0.weight", "mlp.layers.0.bias", "mlp.layers.1.weight", "mlp.layers.1.bias"]
    assert list(enc.state_dict()) == ["hash_table"] and list(net.state_dict()) == keys
    assert enc.get_out_dim() == 10 and [n for n, _ in enc.named_buffers()] == []
    # a CPU tensor reaches the op and is refused there: there is no CPU path (before this forward existed: nn.Module's NotImplementedError)
    for m in (enc, net):
        with pytest.raises(_lib.SignerfHipError, match="GPU"):
            m(torch.rand(7, 3))
    assert list(enc.state_dict()) == ["hash_table"] and list(net.state_dict()) == keys and [n for n, _ in net.named_buffers()] == []
    assert torch.equal(enc.scalings(), onf.hash_scalings(5, 16, 128))


def test_mlp_forward_is_the_oracles():
    torch.manual_seed(0)
    mlp = MLP(10, 3, 16, 4)
    x = torch.randn(33, 10)
    params = {"m." + k: v.detach() for k, v in mlp.state_dict().items()}
    assert torch.equal(mlp(x).detach(), onf.mlp_forward(x, params, "m", 3))
    assert float(mlp(x).detach().min()) < 0        # no output activation


def test_tcnn_grid_has_no_trainable_forward():
    enc = HashEncoding(5, 16, 128, 4, implementation="tcnn")
    with pytest.raises(NotImplementedError, match="tiny-cuda-nn"):
        enc(torch.rand(7, 3))
