"""The per-sample reference of the render kernel (tests/render_oracle.py), on the CPU: the fp32 restatement against oracle.nerfacto's own
per-sample colours, weights and outputs; the fp64 restatement against it to fp32 rounding; the condition under which the accumulation carries
information about the density, decided from the reference alone; and the gate itself fed with MUTATED restatements -- one level's features 1 %
off, the cross term of the coefficient form dropped, two exchanged corners, a feature scale left off one level, the density 2^-12 off, one
negated SH component, the geometry features shifted by one, appearance row 0 instead of the mean -- each of which must exceed the limit that
tests/test_gpu_render_samples.py holds the kernels to (the same gate, at the widest factor it uses anywhere).  No GPU."""
import pytest
import torch

import hashgrid_oracle as ho
import normals_oracle as no
import render_oracle as ro
from helpers import onf

ALL = ("torch", None, 1.0, "contract", "piecewise")
TCNN = ("tcnn", None, 1.0, "contract", "piecewise")
# fp32 restatement from q against the oracle's outputs.  The renderers and the colour head are the oracle's operations in the oracle's order
# (bit for bit, asserted below on its own per-sample tensors).  On the torch grid the density side is the oracle's order too
# (hashgrid_oracle.blend is oracle.nerfacto.hash_encode's nesting; a product and its bias): every bit, both widths.  On the tiny-cuda-nn grid
# the blend nests differently (oracle/tcnn_layout.grid_encode): measured over the cases below rgb 2.0e-6 (64-wide) / 7.3e-6 (128-wide),
# accumulation 1.8e-7 / 3.0e-7, expected_depth 2.4e-7 (one ulp of a depth in [1, 2.5)); depth has no density in it.  Limit = 4 x the
# maximum of its grid and width.
RESTATEMENT_LIMIT = {("torch", False): {"rgb": 0.0, "accumulation": 0.0, "depth": 0.0, "expected_depth": 0.0},
                     ("torch", True): {"rgb": 0.0, "accumulation": 0.0, "depth": 0.0, "expected_depth": 0.0},
                     ("tcnn", False): {"rgb": 8e-6, "accumulation": 7.2e-7, "depth": 0.0, "expected_depth": 1e-6},
                     ("tcnn", True): {"rgb": 3e-5, "accumulation": 1.2e-6, "depth": 0.0, "expected_depth": 1e-6}}
# fp64 restatement against the fp32 oracle: outputs of magnitude <= 2.5 (ulp 2.4e-7) behind five layers of width 64 / 128 with weight gains of
# 2-6: 2^-14 allows 2^10 ulps of 1.0 (measured: at most 1.0e-5, rgb of the 128-wide tiny-cuda-nn case).  A wrong TERM is 1e-3 and more (the mutants).
FP32_ROUNDING = 2.0**-14

CASES = [(c, False, "last_sample") for c in ro.all_cases()] + [(ALL, False, "white"), (ALL, True, "last_sample"), (TCNN, True, "last_sample")] + \
        [(("torch", (k,), 1.0, "contract", "piecewise"), True, "last_sample") for k in (0, 9, 15)]


def _id(case):
    c, wide, background = case
    return ro.case_id(c) + ("-wide" if wide else "") + ("-" + background if background != "last_sample" else "")


def _bg(background):
    return None if background == "last_sample" else ro.WHITE


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_restatement_against_the_oracle(case):
    c, wide, background = case
    _, _, params, ocfg, rays = ro.state(c, wide, False, background)
    ref = ro.reference(c, wide, background)
    dbg = ref["oracle"]
    bins = dbg["euclid_bins"]
    assert bins.shape == (no.N_RAYS, 2) and dbg["q"].shape == (no.N_RAYS, 1, 3)
    # same operations in the same order: every bit
    assert torch.equal(ro.colour(params, ocfg, rays["d"], dbg["mlp_out"][:, 0], torch.float32), dbg["rgb_samples"][:, 0])
    comp = ro.composite(dbg["rgb_samples"][:, 0], dbg["density"][:, 0], bins[:, 0:1], bins[:, 1:2], _bg(background))
    assert torch.equal(comp["w"], dbg["weights"][:, 0])
    for k in ro.OUTPUTS:
        assert torch.equal(comp[k], ref["ref32"][k]), k
    # from q on: the oracle's order on the torch grid (every bit), another nesting of the blend on the tiny-cuda-nn grid
    r32 = ro.sample(params, ocfg, dbg["q"][:, 0], dbg["selector"][:, 0], bins, rays["d"], torch.float32, _bg(background))
    e = {"c": float((r32["c"] - dbg["rgb_samples"][:, 0]).abs().max()), "w": float((r32["w"] - dbg["weights"][:, 0]).abs().max())}
    e.update({k: float((r32[k] - ref["ref32"][k]).abs().max()) for k in ro.OUTPUTS})
    e64 = {k: float((ref["ref32"][k].double() - ref["ref64"][k]).abs().max()) for k in ro.OUTPUTS}
    print(f"{_id(case)}: fp32 restatement - oracle " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()) + " | oracle - fp64 restatement "
          + ", ".join(f"{k} {v:.1e}" for k, v in e64.items()))
    limit = RESTATEMENT_LIMIT[c[0], wide]
    assert e["c"] <= limit["rgb"] and e["w"] <= limit["accumulation"]
    for k in ro.OUTPUTS:
        assert e[k] <= limit[k], k
        assert e64[k] <= FP32_ROUNDING, k
        assert ref["ref64"][k].dtype == torch.float64 and bool(torch.isfinite(ref["ref64"][k]).all()), k
    # what one sample per ray shows
    full = ref["full64"]
    if background == "last_sample":
        assert float((full["rgb"] - full["c"]).abs().max()) <= 2.0**-52          # w c + (1 - w) c
    else:
        assert float((full["rgb"] - (full["w"] * full["c"] + 1 - full["w"])).abs().max()) <= 2.0**-51     # w c + 1 - w
        assert float((full["rgb"] - full["c"]).abs().max()) > 0.1
    assert torch.equal(full["accumulation"], full["w"]) and float(full["w"].min()) > 0 and float(ref["ref32"]["rgb"].std()) > 0.05


def test_coefficient_form_is_the_blend():
    """The form the de-hashed copies hold (and whose cross term a mutant drops) against hashgrid_oracle.blend, in fp64."""
    _, _, params, ocfg, _ = ro.state(ALL)
    grid = no.grid_of(params, ocfg)
    idx, off = no.cells(ro.reference(ALL)["oracle"]["q"][:, 0], grid)
    f, o = ho.gather(grid["table"].double(), idx), off.double()
    assert float((ro.coefficient_blend(f, o) - ho.blend(f, o)).abs().max()) <= 2.0**-50
    assert float((ro.coefficient_blend(f, o, cross=False) - ho.blend(f, o)).abs().max()) > 0.1


@pytest.mark.parametrize("c", [ALL, TCNN], ids=ro.case_id)
def test_one_main_sample_behind_the_proposal_sampler(c):
    """Two proposal levels of (8, 4) samples, one main sample: the oracle renders it, and the restatement at the oracle's q is its colour."""
    _, _, params, ocfg, rays = ro.state(c, proposals=True)
    assert ocfg.num_proposal_iterations == 2 and ocfg.num_proposal_samples_per_ray == ro.PROPOSAL_SAMPLES and ocfg.num_nerf_samples_per_ray == 1
    with torch.no_grad():
        out = onf.get_outputs(params, ocfg, rays["o"], rays["d"], rays["near"], rays["far"], return_debug=True)
    assert all(bool(torch.isfinite(out[k]).all()) for k in ro.OUTPUTS) and float(out["rgb"].std()) > 0.05
    c64, c32 = ro.at_q(c, out["_debug"]["q"][:, 0], rays["d"])
    want = out["_debug"]["rgb_samples"][:, 0]
    e32, e64 = float((c32 - want).abs().max()), float((c64 - want.double()).abs().max())
    print(f"{ro.case_id(c)} behind the proposal sampler: rgb std {float(out['rgb'].std()):.3f}, fp32 restatement at the oracle's q - oracle's colour {e32:.1e}, fp64 {e64:.1e}")
    assert e32 <= RESTATEMENT_LIMIT[c[0], False]["rgb"] and e64 <= FP32_ROUNDING
    assert float((out["rgb"] - want).abs().max()) <= 2.0**-23                       # w c + (1 - w) c, rounded


def test_final_bins_layout_is_the_frame_plans():
    """ops.final_bins_layout (where tests/test_gpu_render_samples.py reads the kernel's own bins) against every recorded plan of a render
    behind the proposal sampler (tests/golden/frame_plans.json: what csrc/sn_frame.h computes)."""
    import json
    import os

    from helpers import GOLDEN
    from signerf_amd import ops

    with open(os.path.join(GOLDEN, "frame_plans.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["nprop"] > 0]
    assert len(cases) >= 5
    seen = 0
    for c in cases:
        lay = ops.final_bins_layout(c["height"], c["width"], c["S"], c["chunk_rays"])
        for call in c["calls"].get("rays_expected_depth", []) + c["calls"].get("rays", []):
            if call.get("ebins") is not None and "tiles_x" in call:
                assert (call["ebins"], call["tiles_x"], call["tiles_y"], 1 << call["tile_w_log2"], 1 << call["tile_h_log2"]) == \
                       (lay["offset"], lay["tiles_x"], lay["tiles_y"], lay["tile_w"], lay["tile_h"]), c["name"]
                seen += 1
    assert seen >= 5


# ---- the accumulation carries information about the density -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_information_condition(case):
    """At sigma delta << 1 the weight is lost in the rounding of 1 - exp(-tau), at >> 1 it saturates at 1 whatever the density is."""
    ref = ro.reference(*case)
    share, w = ro.informative(ref["tau"]), ref["full64"]["w"]
    print(f"{_id(case)}: sigma delta in [{ro.TAU_RANGE[0]}, {ro.TAU_RANGE[1]}] for {100 * share:.1f} % of the samples; w min {float(w.min()):.3f} median "
          f"{float(w.median()):.3f} max {float(w.max()):.4f}, above 0.999: {100 * float((w > 0.999).double().mean()):.1f} %")
    assert share >= ro.MIN_INFORMATIVE


# ---- the gate can fail -------------------------------------------------------------------------------------------------------------------
def _mutant_gate(c, mutant, outputs, wide=False):
    """-> {output: error / limit} of the mutated fp64 restatement; asserts that every one of `outputs` exceeds the gate at F = 8, the
    widest factor any kernel output is held to (render_oracle.gate_factor: 2 for most) -- so it exceeds every limit the GPU tests set."""
    _, _, params, ocfg, rays = ro.state(c, wide)
    ref = ro.reference(c, wide)
    dbg = ref["oracle"]
    got = ro.sample(params, ocfg, dbg["q"][:, 0], dbg["selector"][:, 0], dbg["euclid_bins"], rays["d"], mutant=mutant)
    over = {}
    for k in outputs:
        clean = ro.gate(ref["ref64"][k], ref["ref64"][k], ref["ref32"][k])
        assert clean[0] and clean[1] == 0.0
        ok, e, _, limit = ro.gate(got[k], ref["ref64"][k], ref["ref32"][k])
        over[k] = e / limit
        assert not ok, (k, e, limit)
    over["rmse"] = float(torch.sqrt(torch.mean((got["rgb"] - ref["ref64"]["rgb"]) ** 2)))
    return over


def _fmt(over):
    return ", ".join(f"{k} {v:.0f} x the limit" for k, v in over.items() if k != "rmse")


@pytest.mark.parametrize("level", range(16))
def test_mutants_of_one_level(level):
    """In the level's single-level case and among all 16 levels; both MLPs sit behind the features, so rgb and accumulation both show them."""
    single = ("torch", (level,), 1.0, "contract", "piecewise")
    mutants = [("features x 1.01", ro.Mutant(level=level, feature_factor=1.01)), ("features x 0.99", ro.Mutant(level=level, feature_factor=0.99)),
               ("cross term D dropped", ro.Mutant(level=level, drop_cross_term=True)), ("corners 1 <-> 3", ro.Mutant(level=level, swap_corners=True)),
               ("feat_scale 2 left off", ro.Mutant(level=level, feat_scale=2.0))]
    for name, m in mutants:
        for c in (single, ALL):
            over = _mutant_gate(c, m, ("rgb", "accumulation"))
            line = f"level {level}, {name}, {ro.case_id(c)}: {_fmt(over)}"
            if "x 1.01" in name or "x 0.99" in name:
                # what an image gate at RMSE <= 1e-3 lets through: the whole sample set's rgb RMSE of this mutant
                line += f"; rgb RMSE over the sample set {over['rmse']:.1e}"
            print(line)
            assert min(over["rgb"], over["accumulation"]) > 10


@pytest.mark.parametrize("case", [(ALL, False), (("torch", (4,), 1.0, "contract", "piecewise"), False), (TCNN, False), (ALL, True)],
                         ids=lambda case: ro.case_id(case[0]) + ("-wide" if case[1] else ""))
def test_mutants_behind_the_grid(case):
    c, wide = case
    over = _mutant_gate(c, ro.Mutant(density_factor=1 + 2.0**-12), ("accumulation",), wide)
    print(f"{ro.case_id(c)}: density x (1 + 2^-12): {_fmt(over)}")
    assert over["accumulation"] > 10
    for comp in (1, 6, 15):
        over = _mutant_gate(c, ro.Mutant(flip_sh=comp), ("rgb",), wide)
        print(f"{ro.case_id(c)}: SH component {comp} negated: {_fmt(over)}")
        assert over["rgb"] > 100
    for name, m in (("colour head fed h[:, 0:15]", ro.Mutant(shifted_geo=True)), ("appearance row 0 instead of the mean", ro.Mutant(appearance_row_0=True))):
        over = _mutant_gate(c, m, ("rgb",), wide)
        print(f"{ro.case_id(c)}: {name}: {_fmt(over)}")
        assert over["rgb"] > 100


def test_mutants_of_a_tcnn_level():
    for level in (0, 1, 2, 15):
        for c in (("tcnn", (level,), 1.0, "contract", "piecewise"), TCNN):
            for name, m in (("features x 1.01", ro.Mutant(level=level, feature_factor=1.01)), ("corners 1 <-> 3", ro.Mutant(level=level, swap_corners=True))):
                over = _mutant_gate(c, m, ("rgb", "accumulation"))
                print(f"tiny-cuda-nn level {level}, {name}, {ro.case_id(c)}: {_fmt(over)}")
                assert min(over["rgb"], over["accumulation"]) > 10
