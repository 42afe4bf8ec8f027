"""The render kernels (csrc/sn_main.h sn_render_main_kernel, csrc/sn_wide_kernels.h sn_wide_field_main_kernel) per SAMPLE and per
hash LEVEL against the fp64 restatement of tests/render_oracle.py.

The stage kernel that ops.field_forward runs reads the uploaded table at a world position; the render kernel reads de-hashed copies in
bilinear-coefficient form (levels 0-8), plain copies (9-10), hashed rows (11-15) and, behind the proposal sampler, the x-paired tables, carries
the feature scale inside the copies, takes its positions from its own position maps and composites with its own exponential.  Every other
value test of it is an image gate, in which one level is a sixteenth of the signal.  Here a ray has ONE main sample
(num_nerf_samples_per_ray = 1, per-ray nears / fars), so rgb is that sample's colour (last_sample background) and accumulation its weight
1 - exp(-sigma delta), and the hash table is zeroed but for one level (that level's read path alone in front of both MLPs) or two (their
relative factor: scal[l], the feature scale).  The same 4165 rays as tests/test_gpu_normals_samples.py serve every case (65 waves and 5 lanes;
contraction branch, q within 1e-6 of 0 and 1, exact lattice points); no sample is excluded.

A. behind the uniform sampler (MODE 0) through Model.get_outputs: rgb, accumulation, depth, expected_depth against the restatement at the
   oracle's own q and bins; e_ref32 is the fp32 oracle's error on the same rays.
B. behind the proposal sampler (MODE 1: two proposal levels of (8, 4) samples, the 49 x 85 frame): rgb against the restatement at the
   kernel's own q; e_ref32 is the fp32 restatement's error at that same q.  (The exponential and the compositing are A's code.)
C. the 128-wide fields, A and B.
The instrumented kernels exist for the torch grid with the default copies only.  Every B case therefore takes q from the production launch:
the final bins the proposal kernel left in the workspace (ops.render_with_final_bins), through the main kernel's own position map
(ops.sample_positions); where the instrumented launch exists, the q it dumps must be that q, every bit.

Gate (render_oracle.gate): max |kernel - ref64| <= F x max |oracle32 - ref64| + 1 ulp of the largest output, over all 4165 samples.  F is the
project's 2 (render_oracle.gate_factor) for every output of the exact-fp32 cases (measured: at most 1.65) and for depth and expected_depth
everywhere (1.00); it is 8 for the rgb and the accumulation of the fp16x2 cases alone, whose ratios (up to 5.3 and 6.4) DESIGN.md K1 explains
from the code.  tests/test_render_oracle_host.py shows that a 1 % error of any level's features, a dropped cross term, exchanged corners, a
feature scale left off, a density 2^-12 off and three wrong colour-head inputs all exceed the limit at F = 8.  Every case prints its figures
before it asserts; DESIGN.md K1 holds the table."""
import warnings

import pytest
import torch

import normals_oracle as no
import render_oracle as ro
from signerf_amd import RayBundle, _lib, ops
from signerf_amd.nerfacto import PRECISIONS

pytestmark = pytest.mark.gpu
N_DENSE = {0: 11, 9: 9, -1: 0}     # config.dense_levels -> de-hashed copies of the main grid
ALL = ("torch", None, 1.0, "contract", "piecewise")
TCNN = ("tcnn", None, 1.0, "contract", "piecewise")
_MODELS = {}


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(gpu):
    """A device error ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize(gpu)
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _torch(levels, scale=1.0):
    return ("torch", levels, scale, "contract", "piecewise")


def _levels_id(levels):
    return "all" if levels is None else "L" + "+".join(str(k) for k in levels)


def _model(gpu, c, precision="fp32", dense_levels=0, wide=False, proposals=False, background="last_sample"):
    """One model per (grid, position map, sampler, copy budget, width, sampler depth, background), re-used across cases by loading the
    case's state dict -> (model, rays)."""
    impl, _, _, kind, sampler = c
    _, sd, _, _, rays = ro.state(c, wide, proposals, background)
    key = (impl, kind, sampler, dense_levels, wide, proposals, background, str(gpu))
    if key not in _MODELS:
        _MODELS[key] = ro.config(impl, kind, sampler, wide, proposals, background, dense_levels=dense_levels).setup().to(gpu).eval()
    model = _MODELS[key]
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    model.config.precision = precision
    return model, rays


def _bundle(rays, gpu, shape=None):
    t = {k: rays[k].to(gpu) for k in ("o", "d", "near", "far")}
    if shape is not None:
        t = {k: v.view(*shape, v.shape[-1]) for k, v in t.items()}
    return RayBundle(origins=t["o"], directions=t["d"], pixel_area=torch.ones_like(t["near"]), nears=t["near"], fars=t["far"])


def _instantiation(model, c, precision, dense_levels, wide):
    """The arithmetic that was asked for, the copies that were asked for."""
    assert _lib.load().sn_effective_precision(model._handle, PRECISIONS[precision], 0) == PRECISIONS[precision], "the render kernel changed precision"
    if wide:
        assert model.effective_precision == "fp32" and ops.debug_layout(model)["n_dense"] == 0
    elif c[0] == "torch":
        assert ops.debug_layout(model)["n_dense"] == N_DENSE[dense_levels]


def _render_a(gpu, c, precision="fp32", dense_levels=0, wide=False, background="last_sample", frame=False):
    """-> ({output: [N,C] on the CPU}, the case's reference, the arithmetic that ran)."""
    model, rays = _model(gpu, c, precision, dense_levels, wide, False, background)
    if frame:
        out = model.get_outputs_for_camera_ray_bundle(_bundle(rays, gpu, no.FRAME))
    else:
        out = model.get_outputs(_bundle(rays, gpu))
    assert "normals" not in out                        # the render kernel alone
    got = {k: out[k].reshape(no.N_RAYS, -1).cpu() for k in ro.OUTPUTS}
    _instantiation(model, c, precision, dense_levels, wide)
    return got, ro.reference(c, wide, background), "fp32" if wide else precision


def _gate(name, got, ref64, ref32, outputs, precision):
    """Every output at the factor of its arithmetic (render_oracle.gate_factor: 2, and 8 for the rgb and accumulation of fp16x2)."""
    results = []
    for k in outputs:
        assert got[k].shape == ref64[k].shape and got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all()), k
        factor = ro.gate_factor(precision, k)
        ok, e, e_ref, limit = ro.gate(got[k], ref64[k], ref32[k], factor)
        print(f"{name}: {k}: e_hip {e:.2e} e_ref32 {e_ref:.2e} F {factor} limit {limit:.2e} ratio {e / e_ref:.2f}")
        results.append((k, ok, e, limit))
    for k, ok, e, limit in results:
        assert ok, f"{name}: {k}: {e:.3e} > {limit:.3e}"
    return results


def _check_a(name, got, ref, precision):
    return _gate(name, got, ref["ref64"], ref["ref32"], ro.OUTPUTS, precision)


def _render_b(gpu, c, precision="fp32", dense_levels=0, wide=False):
    """-> (rgb [N,3], q [N,3], d [N,3]).  q is the main kernel's own: its position map (sn_sample_q_fast; the strict sn_sample_q in the wide
    kernel) at the bins the proposal kernel handed it.  Where the instrumented kernels exist (torch grid, default copies) they must equal
    the production ones bit for bit, and the q they dump must be that q."""
    model, rays = _model(gpu, c, precision, dense_levels, wide, True)
    bundle = _bundle(rays, gpu, no.FRAME)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # the "fp16x2 renders as fp32" notice of a wide handle
        prod, bins = ops.render_with_final_bins(model, bundle)
        again = model.get_outputs_for_camera_ray_bundle(bundle)
    for k in ro.OUTPUTS:
        assert torch.equal(prod[k], again[k]), k
    _instantiation(model, c, precision, dense_levels, wide)
    assert bool(torch.isfinite(bins).all()) and bool((bins[:, 1] > bins[:, 0]).all())
    assert bool((bins[:, 0].cpu() >= rays["near"][:, 0] * (1 - 1e-6)).all()) and bool((bins[:, 1].cpu() <= rays["far"][:, 0] * (1 + 1e-6)).all())
    q = ops.sample_positions(rays["o"].to(gpu), rays["d"].to(gpu), bins[:, 0], bins[:, 1])["strict" if wide else "fast"]
    if c[0] == "torch" and dense_levels == 0 and not wide:
        assert ops.debug_layout(model)["pair_bytes"] > 0           # the hashed levels come from the x-paired tables
        out, dump = ops.render_rays_debug(model, bundle, want=("main_q",))
        for k in ro.OUTPUTS:
            assert torch.equal(out[k], prod[k]), f"{k}: the instrumented kernels differ from the production ones"
        assert torch.equal(dump["main_q"].view(no.N_RAYS, 3).view(torch.int32), q.view(torch.int32)), "the dumped q is not the position map at the kept bins"
    q = q.cpu()
    assert bool(torch.isfinite(q).all()) and float(q.min()) >= 0 and float(q.max()) < 1
    return prod["rgb"].reshape(no.N_RAYS, 3).cpu(), q, rays["d"]


def _check_b(name, rgb, q, d, c, wide=False, precision="fp32"):
    c64, c32 = ro.at_q(c, q, d, wide)
    return _gate(name, {"rgb": rgb}, {"rgb": c64}, {"rgb": c32}, ("rgb",), precision)


# ---- A: behind the uniform sampler ----------------------------------------------------------------------------------------------------------
def test_positions_are_the_oracles_bit_for_bit(gpu):
    """The exact position map of the production instantiation (csrc/sn_device.h sn_sample_q_exact) and the strict one of the ALT
    instantiations at the oracle's own bins: the oracle's q, every bit -- the per-sample comparison stands on it."""
    rays, dbg = ro.state(ALL)[4], ro.reference(ALL)["oracle"]
    got = ops.sample_positions(rays["o"].to(gpu), rays["d"].to(gpu), dbg["euclid_bins"][:, 0].to(gpu), dbg["euclid_bins"][:, 1].to(gpu))
    for k in ("exact", "strict"):
        assert torch.equal(got[k].cpu().view(torch.int32), dbg["q"][:, 0].view(torch.int32)), k


@pytest.mark.parametrize("impl,precision,dense_levels,kind,sampler", [
    ("torch", "fp32", 0, "contract", "piecewise"), ("torch", "fp32", 9, "contract", "piecewise"), ("torch", "fp32", -1, "contract", "piecewise"),
    ("torch", "fp16x2", 0, "contract", "piecewise"), ("torch", "fp16x2", 9, "contract", "piecewise"), ("torch", "fp16x2", -1, "contract", "piecewise"),
    ("tcnn", "fp32", 0, "contract", "piecewise"), ("tcnn", "fp16x2", 0, "contract", "piecewise"),
    ("torch", "fp32", 0, "box", "piecewise"), ("torch", "fp32", 0, "contract", "uniform")])      # the last two: the ALT instantiations
def test_all_levels_every_instantiation(gpu, impl, precision, dense_levels, kind, sampler):
    c = (impl, None, 1.0, kind, sampler)
    _check_a(f"{ro.case_id(c)} {precision} dense_levels={dense_levels}", *_render_a(gpu, c, precision, dense_levels))


@pytest.mark.parametrize("level", range(16))
def test_one_level_alone(gpu, level):
    """Levels 0-8: bilinear-coefficient copies, 9-10: plain copies, 11-15: hashed rows."""
    c = _torch((level,))
    _check_a(ro.case_id(c), *_render_a(gpu, c))


@pytest.mark.parametrize("pair", no.PAIRS, ids=_levels_id)
def test_two_adjacent_levels(gpu, pair):
    """The relative factor of two levels (scal[l], the feature scale of the copies), every path boundary included."""
    c = _torch(pair)
    _check_a(ro.case_id(c), *_render_a(gpu, c))


@pytest.mark.parametrize("precision,dense_levels", [("fp16x2", 0), ("fp32", -1)])
@pytest.mark.parametrize("levels", no.BOUNDARY, ids=_levels_id)
def test_boundary_cases_in_other_modes(gpu, levels, precision, dense_levels):
    c = _torch(levels)
    _check_a(f"{ro.case_id(c)} {precision} dense_levels={dense_levels}", *_render_a(gpu, c, precision, dense_levels))


@pytest.mark.parametrize("levels", no.TCNN_LEVELS, ids=_levels_id)
def test_tcnn_levels(gpu, levels):
    """Levels 0 and 1 are indexed densely at T = 2^14, 2 and 15 through the hash."""
    c = ("tcnn", levels, 1.0, "contract", "piecewise")
    _check_a(ro.case_id(c), *_render_a(gpu, c))


@pytest.mark.parametrize("precision", ["fp32", "fp16x2"])
def test_tables_of_realistic_magnitude(gpu, precision):
    """Tables x 1e-3 (nerfstudio's initialisation): the conditioned split-precision form is kept (asserted in _instantiation) and holds the gate."""
    c = _torch(None, scale=1e-3)
    _check_a(f"{ro.case_id(c)} {precision}", *_render_a(gpu, c, precision))


def test_white_background(gpu):
    """rgb = w c + 1 - w: the weight enters the colour."""
    got, ref, precision = _render_a(gpu, ALL, background="white")
    assert float((ref["ref64"]["rgb"] - ref["full64"]["c"]).abs().max()) > 0.1
    _check_a(f"{ro.case_id(ALL)} white background", got, ref, precision)


def test_frame_shape(gpu):
    """The same rays as a 49 x 85 frame (8x8 tiles, ragged on both edges) through get_outputs_for_camera_ray_bundle: the flat bundle's bits."""
    flat, ref, precision = _render_a(gpu, ALL)
    frame, _, _ = _render_a(gpu, ALL, frame=True)
    for k in ro.OUTPUTS:
        assert torch.equal(flat[k], frame[k]), k
    _check_a(f"{ro.case_id(ALL)} as a {no.FRAME[0]}x{no.FRAME[1]} frame", frame, ref, precision)


# ---- B: behind the proposal sampler (the x-paired tables) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16x2"])
@pytest.mark.parametrize("dense_levels", [0, 9, -1])
def test_all_levels_behind_the_proposal_sampler(gpu, dense_levels, precision):
    rgb, q, d = _render_b(gpu, ALL, precision, dense_levels)
    _check_b(f"proposals {ro.case_id(ALL)} {precision} dense_levels={dense_levels}", rgb, q, d, ALL, precision=precision)


@pytest.mark.parametrize("levels", [(k,) for k in range(9, 16)] + [(8, 9), (10, 11)], ids=_levels_id)
def test_levels_behind_the_proposal_sampler(gpu, levels):
    """Plain copies 9-10, the x-paired tables 11-15, and the boundaries coefficient | plain and copy | paired."""
    c = _torch(levels)
    rgb, q, d = _render_b(gpu, c)
    _check_b(f"proposals {ro.case_id(c)}", rgb, q, d, c)


def test_tcnn_behind_the_proposal_sampler(gpu):
    rgb, q, d = _render_b(gpu, TCNN)
    _check_b(f"proposals {ro.case_id(TCNN)}", rgb, q, d, TCNN)


# ---- C: the 128-wide fields -------------------------------------------------------------------------------------------------------------------
def _wide_a(gpu, c):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return _render_a(gpu, c, wide=True)


@pytest.mark.parametrize("c", [ALL, TCNN, _torch((0,)), _torch((9,)), _torch((15,))], ids=ro.case_id)
def test_wide_field(gpu, c):
    _check_a(f"wide {ro.case_id(c)}", *_wide_a(gpu, c))


def test_wide_field_behind_the_proposal_sampler(gpu):
    rgb, q, d = _render_b(gpu, ALL, wide=True)
    _check_b(f"proposals wide {ro.case_id(ALL)}", rgb, q, d, ALL, wide=True)
