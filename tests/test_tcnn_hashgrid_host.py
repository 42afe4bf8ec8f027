"""Trainable tiny-cuda-nn grid, CPU side: the restatement tests/tcnn_hashgrid_oracle.py against ``oracle.tcnn_layout.grid_encode`` bit for
bit, the gradient formulas the kernels implement against ``torch.autograd`` in fp64, the level geometry the kernels compile
(``sn_hashgrid_tcnn_levels``, host only) against ``grid_meta`` and ``tcnn_import.grid_level_table``, the companion C header
signerf_amd/include/signerf_hip_hashgrid_tcnn.h against the binding, the library's exports and its argument refusals (in a child process: nothing is
launched), and what ``config.training_tcnn`` switches at set-up.  No GPU."""
import ctypes as C
import os

import pytest
import torch

import hashgrid_oracle as ho
import tcnn_hashgrid_oracle as to
from abi_helpers import c99_probe, declared, exported, refusal_sweep
from helpers import ROOT, small_config
from oracle import tcnn_layout as tl
from signerf_amd import _lib, hashgrid, tcnn_import
from signerf_amd.nerfacto import MLP, HashEncoding

D = torch.float64
SHAPES = [(8, 13, 4, 64), (6, 12, 2, 40), (16, 19, 16, 2048), (5, 17, 16, 128), (16, 10, 16, 2048), (1, 9, 8, 8)]   # (L, log2_T, base, max)


def _meta(L, log2_T, base, mx, F=2):
    return tl.grid_meta(L, base, mx, log2_T, F)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,log2_T,base,mx,F", [s + (2,) for s in SHAPES] + [s + (4,) for s in SHAPES if s[1] <= 13])
def test_restatement_in_fp32_is_the_oracle_bit_for_bit(L, log2_T, base, mx, F):
    meta = _meta(L, log2_T, base, mx, F)
    q = to.points(257, seed=L + log2_T, meta=meta)
    table = to.table(meta, F, seed=7)
    enc, idx = to.encode(q, table, meta, torch.float32)
    want = tl.grid_encode(q, to.flat_rows(table, meta), meta)
    assert enc.shape == (257, L * F) and torch.equal(enc.view(torch.int32), want.view(torch.int32))
    T = 1 << log2_T
    assert torch.equal(idx // T, torch.arange(L).view(1, L, 1).expand_as(idx))
    for l, n in enumerate(to.level_rows(meta)):
        assert int((idx[:, l] - l * T).max()) < n
    assert torch.equal(to.flat_rows(to.uniform_table(to.flat_rows(table, meta), meta), meta), to.flat_rows(table, meta))
    assert bool(to.in_domain(q, meta).all())


def test_what_the_shapes_cover():
    """What the shapes of tests/test_gpu_tcnn_hashgrid.py exercise: which levels are dense, and where the dense index wraps past n_l for q
    in [0, 1]."""
    def wraps(meta):
        q = to.points(4096, seed=1, meta=meta)
        _, _, x = to.cells(q, meta)
        out = []
        for l in range(meta.num_levels):
            r, n = meta.resolutions[l], to.level_rows(meta)[l]
            c = torch.floor(x[:, l]).to(torch.int64) + 1
            out.append(meta.dense[l] and int((c[:, 0] + c[:, 1] * r + c[:, 2] * r * r).max()) >= n)
        return out

    m = _meta(8, 13, 4, 64)
    assert m.dense == [True] * 5 + [False] * 3 and [l for l, hit in enumerate(wraps(m)) if hit] == [0, 1, 2, 4]
    m = _meta(6, 12, 2, 40)
    assert m.dense == [True] * 4 + [False] * 2 and m.resolutions[0] == 2
    assert _meta(1, 9, 8, 8).dense == [True] and not any(_meta(16, 10, 16, 2048).dense)
    assert sum(_meta(16, 19, 16, 2048).dense) == 5 and sum(_meta(5, 17, 16, 128).dense) == 3


# ---- the gradients the kernels form, against autograd in fp64 --------------------------------------------------------------------------
@pytest.mark.parametrize("L,log2_T,base,mx", [s for s in SHAPES if s[1] <= 13])
@pytest.mark.parametrize("F", [1, 2, 8])
def test_gradient_formulas_equal_autograd(L, log2_T, base, mx, F):
    meta = _meta(L, log2_T, base, mx, F)
    q, table = to.points(257, seed=3, meta=meta), to.table(meta, F, seed=5)
    g = torch.randn(257, L * F, generator=torch.Generator().manual_seed(3), dtype=D)
    want_t, want_q = to.grads(q, table, meta, g, D)
    idx, w, _ = to.cells(q, meta)
    got_t = to.grad_table_formula(idx, w, g, table.shape[0])
    got_q = to.grad_q_formula(ho.gather(table.to(D), idx), w, meta, g)      # the torch-path derivative on the corners in nerfstudio's order
    assert float((got_t - want_t).abs().max()) <= 1e-12 * float(want_t.abs().max())
    assert float((got_q - want_q).abs().max()) <= 1e-12 * float(want_q.abs().max())
    cw = to.corner_weights(w.double())
    assert float(cw.min()) >= 0.0 and float(cw.max()) <= 1.0 and float((cw.sum(-1) - 1).abs().max()) <= 1e-14
    n, A = to.contributions(idx, w, g, table.shape[0])
    assert int(n[:, 0].sum()) == 257 * L * 8 and bool((A[n == 0] == 0).all()) and bool((n[~to.used_rows(meta)] == 0).all())
    assert bool((got_t.abs() <= A * (1 + 1e-12)).all())


# ---- the level geometry the kernels compile --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,log2_T,base,mx", SHAPES)
def test_level_query_equals_grid_meta_and_the_importer(built_lib, L, log2_T, base, mx):
    meta = _meta(L, log2_T, base, mx)
    enc = HashEncoding(L, base, mx, log2_T, implementation="tcnn") if log2_T <= 13 else None
    s = enc.scalings() if enc is not None else to.scalings(meta)
    assert torch.equal(s, to.scalings(meta))
    res, rows, dense = hashgrid.tcnn_levels(s.tolist(), log2_T)
    assert res == meta.resolutions and rows == to.level_rows(meta) and dense == meta.dense
    imp_res, imp_offs = tcnn_import.grid_level_table(L, base, mx, log2_T)
    assert res == imp_res and rows == [imp_offs[l + 1] - imp_offs[l] for l in range(L)]
    assert all(r <= 256 for r, d in zip(res, dense) if d)


def test_level_query_is_defined_for_every_scale(built_lib):
    """r up to 256 is dense at T = 2^24; whatever a scale holds, n stays in [8, T] (no input addresses outside a slot)."""
    inf, nan = float("inf"), float("nan")
    res, rows, dense = hashgrid.tcnn_levels([255.0, 254.5, 255.5, 0.0, -3.0, 1e30, inf, nan, 0.25], 24)
    assert res[:3] == [256, 256, 257] and rows[:3] == [1 << 24] * 3 and dense[:3] == [True, True, False]
    assert res[3:] == [1, 1, (1 << 20) + 1, (1 << 20) + 1, 1, 2] and rows[3:] == [8, 8, 1 << 24, 1 << 24, 8, 8]
    assert dense[3:] == [True, True, False, False, True, True]
    res, rows, dense = hashgrid.tcnn_levels([1.0, 3.0], 1)
    assert rows == [2, 2] and dense == [False, False]
    lib = _lib.load()
    for bad in ((0, 10), (33, 10), (4, 0), (4, 25)):
        assert lib.sn_hashgrid_tcnn_levels((C.c_float * 40)(), bad[0], bad[1], None, None, None) == _lib.SN_ERR_INVALID
        assert b"sn_hashgrid_tcnn_levels" in lib.sn_last_error(None)
    assert lib.sn_hashgrid_tcnn_levels(None, 4, 10, None, None, None) == _lib.SN_ERR_INVALID
    assert lib.sn_hashgrid_tcnn_levels((C.c_float * 4)(), 4, 10, None, None, None) == _lib.SN_OK


# ---- the companion C header ------------------------------------------------------------------------------------------------------------
NAMES = ["sn_hashgrid_tcnn_abi_version", "sn_hashgrid_tcnn_backward", "sn_hashgrid_tcnn_forward", "sn_hashgrid_tcnn_levels"]
KERNELS = ["sn_hashgrid_forward_kernel", "sn_hashgrid_backward_table_kernel", "sn_hashgrid_backward_input_kernel"]


HEADER = os.path.join(_lib.EXTENSION_DIR, "signerf_hip_hashgrid_tcnn.h")


def test_header_binding_exports_version_and_build_agree(built_lib):
    """What tests/test_cabi.py holds for every header of include/, for this header of the package's own include directory: an entry of
    _lib.EXTENSIONS, outside _lib.REGISTRY and include/, which that test holds against each other."""
    from signerf_amd import build

    h = _lib.header("hashgrid_tcnn")
    assert h in _lib.EXTENSIONS and h not in _lib.REGISTRY and not set(h.functions) & set(_lib.functions())
    assert h.file == os.path.basename(HEADER) and h.file not in os.listdir(os.path.join(ROOT, "include")) and not h.recorded
    assert declared(HEADER) == sorted(h.functions) == NAMES
    assert not sorted(set(h.functions) - exported(built_lib))
    assert h.version_fn in h.functions and h.version_macro == "SN_HASHGRID_TCNN_ABI_VERSION"
    assert _lib.load().sn_hashgrid_tcnn_abi_version() == h.version == 1
    assert os.path.join("..", "include", h.file) in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "..", "include", h.file))
    lib = _lib.load()
    for name, (res, args) in h.functions.items():          # load() bound the extension's entry points too
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    blob = open(built_lib, "rb").read()
    for k in KERNELS:
        for F in (1, 2, 4, 8):     # the grid's instantiations, beside the torch-path ones tests/test_hashgrid_host.py looks for
            tag = ("_Z%d%sILi%dE" % (len(k), k, F)).encode()
            assert any(tag + mid + b"12SnHgTcnnGridE" in blob for mid in (b"", b"Lb0E", b"Lb1E")), (k, F)


def test_load_refuses_a_library_of_another_version(built_lib, monkeypatch):
    h = _lib.header("hashgrid_tcnn")
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "EXTENSIONS", tuple(x._replace(version=x.version + 7) if x.key == h.key else x for x in _lib.EXTENSIONS))
    with pytest.raises(_lib.SignerfHipError, match=f"reports {h.version_macro} 1, this binding was written for 8: rebuild the library"):
        _lib.load()
    assert _lib._lib is None


def test_header_compiles_as_c99(tmp_path):
    assert c99_probe(tmp_path, ("signerf_hip_hashgrid.h", HEADER), "%d %d %d",
                     "SN_HASHGRID_TCNN_ABI_VERSION, SN_HASHGRID_TCNN_MAX_LEVELS, SN_HASHGRID_TCNN_MAX_LOG2_T") == ["1", "32", "24"]


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
    return done(lib.sn_hashgrid_tcnn_forward(q, table, s, n, L, T, F, enc, idx, N), "sn_hashgrid_tcnn_forward")
def bw(q=P, table=P, s=P, g=P, n=4, L=16, T=19, F=2, gt=P, gq=P):
    return done(lib.sn_hashgrid_tcnn_backward(q, table, s, g, n, L, T, F, gt, gq, N), "sn_hashgrid_tcnn_backward")
calls = {"abi": lambda: "%d:text" % lib.sn_hashgrid_tcnn_abi_version()}
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


def test_entry_points_refuse_bad_arguments_before_the_device(built_lib):
    """The sibling header's sweep on this header's entry points: SN_ERR_INVALID with the entry point's OWN name in sn_last_error; N = 0 is
    SN_OK without a launch.  In a child process -- a crash would be a segfault -- and host-only."""
    got = refusal_sweep(_SWEEP)
    want = {k: ("0:text" if k.startswith("ok_") else "1:text") for k in got}
    want["abi"] = "1:text"
    assert len(got) == 52 and got == want


# ---- the Python surface and the config switch ------------------------------------------------------------------------------------------
def test_python_surface_refuses_before_the_device():
    meta = _meta(5, 4, 16, 128)
    q, table, s = torch.zeros(4, 3), torch.zeros(5 << 4, 2), to.scalings(meta)
    with pytest.raises(ValueError, match="grid"):
        hashgrid.hash_encode(q, table, s, 4, grid="dense")
    for fn in (hashgrid.hash_encode, hashgrid.hash_corner_indices):
        with pytest.raises(_lib.SignerfHipError, match="GPU"):
            fn(q, table, s, 4, grid="tcnn")
        with pytest.raises(TypeError, match="fp32"):
            fn(q.double(), table, s, 4, grid="tcnn")
    with pytest.raises(_lib.SignerfHipError, match="GPU"):
        hashgrid.hash_encode_backward(q, table, s, 4, torch.zeros(4, 10), want_grad_q=True, grid="tcnn")


def test_without_training_tcnn_a_tcnn_model_refuses_to_train():
    from signerf_amd import Frustums, RaySamples
    from signerf_amd.nerfacto import _training_q

    enc = HashEncoding(5, 16, 128, 4, implementation="tcnn")
    assert enc.trainable_tcnn is False and "trainable_tcnn" not in enc.__dict__
    with pytest.raises(NotImplementedError, match="tiny-cuda-nn"):
        enc(torch.rand(7, 3))
    with pytest.raises(NotImplementedError, match="tiny-cuda-nn"):
        small_config(training_mlp="hip", implementation="tcnn").setup()
    model = small_config(implementation="tcnn", training_forward=True).setup()
    assert not any(m.trainable_tcnn for m in model.modules() if isinstance(m, HashEncoding))
    z = torch.zeros(2, 3, 1)
    rs = RaySamples(Frustums(torch.zeros(2, 3, 3), torch.ones(2, 3, 3), z, z + 1, z + 1))
    with pytest.raises(NotImplementedError, match="tiny-cuda-nn"):
        _training_q(model, rs)
    with pytest.raises(NotImplementedError, match="tiny-cuda-nn"):
        model.proposal_networks[0].get_density_training(rs)
    # the switch changes nothing on a torch-path model
    torch_model = small_config(training_tcnn=True).setup()
    assert not any(m.trainable_tcnn for m in torch_model.modules() if isinstance(m, HashEncoding))


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_with_training_tcnn_the_model_sets_up_on_the_hip_mlp(precision):
    cfg = small_config(implementation="tcnn", training_tcnn=True, training_forward=True, training_mlp="hip", training_mlp_precision=precision)
    model = cfg.setup()
    grids = [m for m in model.modules() if isinstance(m, HashEncoding)]
    assert len(grids) == 3 and all(m.trainable_tcnn and m.implementation == "tcnn" for m in grids)
    stacks = [m for m in model.modules() if isinstance(m, MLP)]
    assert all(m.implementation == "hip" and m.precision == precision for m in stacks)
    assert not any("trainable" in k for k in model.state_dict())                      # a plain attribute: the state dict is what it was
    with pytest.raises(_lib.SignerfHipError, match="GPU"):                            # the op is reached, and has no CPU path
        grids[0](torch.rand(7, 3))
    assert torch.equal(grids[0].scalings(), to.scalings(tl.grid_meta(cfg.num_levels, cfg.base_res, cfg.max_res, cfg.log2_hashmap_size)))
    with pytest.raises(NotImplementedError, match="training_normals"):
        small_config(implementation="tcnn", training_tcnn=True, training_normals=True).setup()
