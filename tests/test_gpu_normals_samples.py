"""The normals kernel (csrc/sn_normals.h) per SAMPLE and per hash LEVEL against the fp64 restatement of tests/normals_oracle.py.

Every other test of this kernel is an image gate on composited, renormalised normals, which the fine levels dominate: a 10 % slope error of
levels 0-2 or a dropped zero-offset factor passes them.  Here a ray has ONE sample (num_nerf_samples_per_ray = 1, no proposal nets, per-ray
nears / fars), so "normals" is that sample's (-g / |g| + 1) / 2, and the hash table is zeroed but for one level (that level's slope path alone
decides the direction) or two (their relative factor: scal[l] * inv_scale, the feature scale of the copies).  The same 4165 rays serve every
case (65 waves and 5 lanes; contraction branch, q within 1e-6 of 0 and 1, lattice points with offsets of exactly 0 on 1, 2 and 3 axes).

Gate (tests/hashgrid_oracle.gate): max |kernel - ref64| <= GATE_FACTOR x max |oracle32 - ref64| + 1 ulp of the largest output, over the
samples no tie decides (normals_oracle.ambiguous: at most 2 %); the samples exactly on a voxel face are part of it and reported apart.  The
host tests (tests/test_normals_oracle_host.py) show that a 1 % slope error of any level and a dropped zero-offset rule exceed this limit
90 times and more.  GATE_FACTOR is 8: the largest measured e_hip / e_ref32 is 7.06, decided by the worst-conditioned sample of its case
(normals_oracle.GATE_FACTOR; DESIGN.md K3 holds the figures of every case, which are printed here before they are asserted)."""
import pytest
import torch

import normals_oracle as no
from signerf_amd import RayBundle, _lib, ops
from signerf_amd.nerfacto import PRECISIONS

pytestmark = pytest.mark.gpu
N_DENSE = {0: 11, 9: 9, -1: 0}     # config.dense_levels -> de-hashed copies of the main grid (the normals kernel reads 11 or none)
_MODELS = {}


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(gpu):
    """A device error ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize(gpu)
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _model(gpu, impl, kind, sampler, dense_levels, sd):
    """One model per (grid, position map, sampler, copy budget), re-used across cases by loading the case's state dict."""
    key = (impl, kind, sampler, dense_levels, str(gpu))
    if key not in _MODELS:
        _MODELS[key] = no.config(impl, kind, sampler, dense_levels=dense_levels).setup().to(gpu).eval()
    model = _MODELS[key]
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    return model


def _bundle(rays, gpu, shape=None):
    t = {k: rays[k].to(gpu) for k in ("o", "d", "near", "far")}
    if shape is not None:
        t = {k: v.view(*shape, v.shape[-1]) for k, v in t.items()}
    return RayBundle(origins=t["o"], directions=t["d"], pixel_area=torch.ones_like(t["near"]), nears=t["near"], fars=t["far"])


def _render(gpu, c, precision="fp32", dense_levels=0, frame=False):
    impl, _, _, kind, sampler = c
    sd, _, _, rays, ref = no.case(*c)
    model = _model(gpu, impl, kind, sampler, dense_levels, sd)
    model.config.precision = precision
    if frame:
        out = model.get_outputs_for_camera_ray_bundle(_bundle(rays, gpu, no.FRAME))
    else:
        out = model.get_outputs(_bundle(rays, gpu))
    got = {k: out[k].reshape(-1, 3).cpu() for k in ("normals", "pred_normals")}
    # the instantiation: the arithmetic that was asked for, the copies that were asked for
    assert _lib.load().sn_effective_precision(model._handle, PRECISIONS[precision], 1) == PRECISIONS[precision], "the normals kernel changed precision"
    if impl == "torch":
        assert ops.debug_layout(model)["n_dense"] == N_DENSE[dense_levels]
    return got, rays, ref


def _check(name, got, rays, ref):
    n = no.N_RAYS
    keep, face = ref["keep"], ref["exact_face"] & ref["keep"]
    excluded = int((~keep).sum())
    assert excluded <= no.MAX_EXCLUDED * n and float(ref["weights"][keep].min()) >= no.MIN_WEIGHT
    # pred_normals: the oracle's fp32 sin(2 pi 2^k p) has no digit left at |p| ~ 1e6 (its e_ref32 there is 0.1-0.4, and a limit made of it
    # would hold nothing), while the kernel reduces the argument exactly (v_fract of an exact power-of-two multiple): e_ref32 is taken on the
    # other rows, and the far rows are held to the limit it gives like every other sample
    near = keep & ~rays["far_rows"]
    results = []
    for k, ref_rows in (("normals", keep), ("pred_normals", near)):
        assert got[k].shape == (n, 3) and got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all()), k
        _, _, e_ref, limit = no.gate(got[k], ref["ref64"][k], ref["ref32"][k], ref_rows)
        e = float((got[k].double() - ref["ref64"][k])[keep].abs().max())
        print(f"{name}: {k}: e_hip {e:.2e} e_ref32 {e_ref:.2e} limit {limit:.2e} ratio {e / e_ref:.2f} | {int(keep.sum())} compared, "
              f"{excluded} excluded ({int(ref['relu_tie'].sum())} ReLU ties, {int(ref['near_face'].sum())} near a face)")
        results.append((k, e <= limit, e, limit))
    e_face = float((got["normals"].double() - ref["ref64"]["normals"])[face].abs().max()) if bool(face.any()) else 0.0
    e_tie = (got["normals"].double() - ref["ref64"]["normals"])[~keep].abs().max(-1).values
    e_far = float((got["pred_normals"].double() - ref["ref64"]["pred_normals"])[keep & rays["far_rows"]].abs().max()) if bool(rays["far_rows"].any()) else 0.0
    print(f"{name}: exactly on a face: {int(face.sum())} samples, e_hip {e_face:.2e}; of the {excluded} excluded samples {int((e_tie > 1e-4).sum())} differ by more "
          f"than 1e-4; pred_normals at |p| >= 50: e_hip {e_far:.2e}")
    for what, ok, e, limit in results:
        assert ok, f"{name}: {what}: {e:.3e} > {limit:.3e}"
    return results


def _torch(levels, scale=1.0, kind="contract", sampler="piecewise"):
    return ("torch", levels, scale, kind, sampler)


def _levels_id(levels):
    return "all" if levels is None else "L" + "+".join(str(k) for k in levels)


def test_positions_are_the_oracles_bit_for_bit(gpu):
    """The strict position map (csrc/sn_device.h sn_sample_q: the normals kernel's) at the oracle's own bins: the oracle's q, every bit --
    the per-sample comparison below stands on it (a position one ulp off sits in the neighbouring voxel of a fine level)."""
    _, _, _, rays, ref = no.case()
    got = ops.sample_positions(rays["o"].to(gpu), rays["d"].to(gpu), ref["starts"].to(gpu), ref["ends"].to(gpu))
    assert torch.equal(got["strict"].cpu().view(torch.int32), ref["q"].view(torch.int32))


@pytest.mark.parametrize("impl,precision,dense_levels,kind,sampler", [
    ("torch", "fp32", 0, "contract", "piecewise"), ("torch", "fp32", 9, "contract", "piecewise"), ("torch", "fp32", -1, "contract", "piecewise"),
    ("torch", "fp16x2", 0, "contract", "piecewise"), ("torch", "fp16x2", 9, "contract", "piecewise"), ("torch", "fp16x2", -1, "contract", "piecewise"),
    ("tcnn", "fp32", 0, "contract", "piecewise"), ("tcnn", "fp16x2", 0, "contract", "piecewise"),
    ("torch", "fp32", 0, "box", "piecewise"), ("torch", "fp32", 0, "contract", "uniform")])      # the last two: the ALT instantiations
def test_all_levels_every_instantiation(gpu, impl, precision, dense_levels, kind, sampler):
    c = (impl, None, 1.0, kind, sampler)
    got, rays, ref = _render(gpu, c, precision, dense_levels)
    _check(f"{no.case_id(c)} {precision} dense_levels={dense_levels}", got, rays, ref)


@pytest.mark.parametrize("level", range(16))
def test_one_level_alone(gpu, level):
    """Levels 0-8: bilinear-coefficient copies, 9-10: plain copies, 11-15: hashed rows; 0-6 re-gathered in the second pass, 7-15 kept."""
    c = _torch((level,))
    _check(no.case_id(c), *_render(gpu, c))


@pytest.mark.parametrize("pair", no.PAIRS, ids=_levels_id)
def test_two_adjacent_levels(gpu, pair):
    """The relative factor of two levels (a uniform factor on the only live level normalises away), every path boundary included."""
    c = _torch(pair)
    _check(no.case_id(c), *_render(gpu, c))


@pytest.mark.parametrize("precision,dense_levels", [("fp16x2", 0), ("fp32", -1)])
@pytest.mark.parametrize("levels", no.BOUNDARY, ids=_levels_id)
def test_boundary_cases_in_other_modes(gpu, levels, precision, dense_levels):
    c = _torch(levels)
    _check(f"{no.case_id(c)} {precision} dense_levels={dense_levels}", *_render(gpu, c, precision, dense_levels))


@pytest.mark.parametrize("levels", no.TCNN_LEVELS, ids=_levels_id)
def test_tcnn_levels(gpu, levels):
    """Levels 0 and 1 are indexed densely at T = 2^14, 2 and 15 through the hash."""
    c = ("tcnn", levels, 1.0, "contract", "piecewise")
    _check(no.case_id(c), *_render(gpu, c))


@pytest.mark.parametrize("precision", ["fp32", "fp16x2"])
def test_tables_of_realistic_magnitude(gpu, precision):
    """Tables x 1e-3 (nerfstudio's initialisation): the conditioned split-precision form is kept (asserted in _render) and holds the gate."""
    c = _torch(None, scale=1e-3)
    _check(f"{no.case_id(c)} {precision}", *_render(gpu, c, precision))


def test_frame_shape(gpu):
    """The same rays as a 49 x 85 frame (8x8 tiles, ragged on both edges) through get_outputs_for_camera_ray_bundle: the same gate."""
    c = _torch(None)
    flat, rays, ref = _render(gpu, c)
    frame, _, _ = _render(gpu, c, frame=True)
    print("frame against the flat bundle: " + ", ".join(f"{k} {'bit-identical' if torch.equal(flat[k], frame[k]) else 'max |d| %.2e' % float((flat[k] - frame[k]).abs().max())}"
                                                       for k in flat))
    _check(f"{no.case_id(c)} as a {no.FRAME[0]}x{no.FRAME[1]} frame", frame, rays, ref)
