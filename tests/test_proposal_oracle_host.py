"""The per-sample reference of the proposal kernel (tests/proposal_oracle.py), on the CPU.

1. The restatement is the oracle: chain(float32) at the oracle's own prop_q_0 equals oracle.nerfacto.get_outputs bit for bit on every
   level's weights, spacing bins and median depth and on the final euclidean bins -- both grids, contraction / box / uniform sampler, ONE,
   TWO and DENSE.
2. The reference is a reference: e_ref32 = max |chain32 - chain64| of the final bins is at most 1e-4 x the largest bin (a condition that a
   broken fp64 path misses by orders of magnitude -- get_outputs on .double() inputs is 0.1 off --, not a tolerance).
3. The gate can fail: every mutant of proposal_oracle.Mutant, on each net it applies to, moves the final bins of DENSE beyond the limit at
   F = 8, the widest factor in use.  One mutant CANNOT be seen by any output of a render: "+ padding / N dropped".  padding = relu(1e-5 -
   sum(w + histogram_padding)) is exactly 0 whenever N x histogram_padding >= 1e-5, which nerfacto's 0.01 makes true for every ray; the term
   only lives with histogram_padding = 0 on a ray without weight, which no render of this project configures.  It is reported below with
   ratio 0, not dropped; the output that does see it is PDFSampler itself at histogram_padding = 0 (proposal_oracle.padding_case: far beyond
   the limit), which tests/test_gpu_proposal_samples.py asks of ops.pdf_sample -- the stage kernel shares SnPdfNorm with the proposal kernel.
4. Information condition, from the reference alone: on DENSE at most 2 % of the rays pass 0.5 within margin_k = 8 x max |cumsum32_k -
   cumsum64_k| (the rays the GPU tests' median check leaves out), every ray's cumulative weight does cross 0.5, and on TWO the median
   proposal weight exceeds histogram_padding (the weights, not the padding, shape the pdf).
5. ops.final_bins_layout for the GPU tests' frames (49 x 85 and 1 x 4165, S = 16 and 32) against sn_plan_frame through the host-only
   tests/c/frame_plan.cpp client.  No GPU."""
import itertools
import os
import subprocess

import pytest
import torch

import normals_oracle as no
import proposal_oracle as po
from helpers import ROOT

VARIANTS = [("contract", "piecewise"), ("box", "piecewise"), ("contract", "uniform")]
CASES = [po.case(impl, kind, sampler, setting) for impl in ("torch", "tcnn") for kind, sampler in VARIANTS for setting in ("ONE", "TWO", "DENSE")]
CASES.append(po.case("tcnn", setting="TWO", nets="all-dense"))
REFERENCE_CONDITION = 1e-4
DENSE = po.case(setting="DENSE")


def _equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1, 2: the restatement and the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=po.case_id)
def test_restatement_is_the_oracle_and_the_reference_is_a_reference(c):
    _, _, params, ocfg, rays = po.state(c)
    out = po.oracle_outputs(c)
    dbg = out["_debug"]
    r64, r32 = po.references(c)
    n = ocfg.num_proposal_iterations
    assert dbg["prop_q_0"].shape == (no.N_RAYS, ocfg.num_proposal_samples_per_ray[0], 3) and len(r32["levels"]) == n
    for k in range(n):
        lv = r32["levels"][k]
        assert _equal(lv["weights"], dbg[f"prop_weights_{k}"][..., 0]), f"prop_weights_{k}"
        assert _equal(lv["sbins"], dbg[f"prop_sbins_{k}"].contiguous()), f"prop_sbins_{k}"
        assert _equal(lv["median"], out[f"prop_depth_{k}"]), f"prop_depth_{k}"
        assert _equal(lv["q"], dbg[f"prop_q_{k}"]), f"prop_q_{k}"
    assert _equal(r32["ebins"], dbg["euclid_bins"]) and _equal(r32["sbins"], dbg["spacing_bins"])
    # the fp64 chain against it
    assert r64["ebins"].dtype == torch.float64 and bool(torch.isfinite(r64["ebins"]).all())
    e, top = float((r32["ebins"].double() - r64["ebins"]).abs().max()), float(r64["ebins"].abs().max())
    e_w = [float((r32["levels"][k]["weights"].double() - r64["levels"][k]["weights"]).abs().max()) for k in range(n)]
    print(f"{po.case_id(c)}: final bins e_ref32 {e:.2e} (largest bin {top:.3f}, e / top {e / top:.1e}); weights e_ref32 " + ", ".join(f"{v:.1e}" for v in e_w))
    assert 0 < e <= REFERENCE_CONDITION * top
    assert bool((r64["ebins"][:, 1:] > r64["ebins"][:, :-1]).all())
    assert bool((r64["ebins"][:, 0] >= rays["near"][:, 0].double() * (1 - 1e-6)).all()) and bool((r64["ebins"][:, -1] <= rays["far"][:, 0].double() * (1 + 1e-6)).all())


def test_a_dead_ray_is_resampled_uniformly():
    """The chain with a ray's weights zero (what the oracle gives for a NaN origin) is the oracle's, bit for bit, on the other rays and on
    that ray: its pdf is the padding's, its final bins finite."""
    c = po.case(setting="TWO")
    _, _, params, ocfg, rays = po.state(c)
    dead = torch.arange(no.N_RAYS) % 3 == 0
    bad = dict(rays)
    bad["o"] = torch.where(dead[:, None] & (torch.arange(3) == 1), torch.full((), float("nan")), rays["o"])
    from helpers import onf

    with torch.no_grad():
        out = onf.get_outputs(params, ocfg, bad["o"], bad["d"], bad["near"], bad["far"], return_debug=True)
    r32 = po.chain(params, ocfg, rays, out["_debug"]["prop_q_0"], torch.float32, dead=dead)
    assert _equal(r32["ebins"], out["_debug"]["euclid_bins"]) and bool(torch.isfinite(r32["ebins"]).all())
    assert float(out["_debug"]["prop_weights_0"][dead].abs().max()) == 0 and float(out["_debug"]["prop_weights_1"][dead].abs().max()) == 0
    for k in range(2):
        assert _equal(r32["levels"][k]["median"], out[f"prop_depth_{k}"])
    clean = po.references(c)[1]
    assert _equal(r32["ebins"][~dead], clean["ebins"][~dead])


# ---- 3: the gate can fail ---------------------------------------------------------------------------------------------------------------------
def _level_mutants(net, level):
    return [(f"net {net} level {level}: features x 1.01", po.Mutant(net=net, level=level, feature_factor=1.01)),
            (f"net {net} level {level}: cross term D dropped", po.Mutant(net=net, level=level, drop_cross_term=True)),
            (f"net {net} level {level}: corners 1 <-> 3", po.Mutant(net=net, level=level, swap_corners=True)),
            (f"net {net} level {level}: feature scale 2 left off", po.Mutant(net=net, level=level, feat_scale=2.0))]


def _net_mutants(net):
    return [(f"net {net}: density x (1 + 2^-9)", po.Mutant(net=net, density_factor=1 + 2.0**-9)),
            (f"net {net}: relu(x) -> x / 2", po.Mutant(net=net, drop_abs_half=True)),
            (f"net {net}: bias of hidden unit 5 dropped", po.Mutant(net=net, drop_hidden_bias=5)),
            (f"net {net}: histogram_padding not added", po.Mutant(net=net, no_histogram_padding=True)),
            (f"net {net}: transmittance includes the sample's own tau", po.Mutant(net=net, inclusive_transmittance=True)),
            (f"net {net}: u without + 1 / (2 (M + 1))", po.Mutant(net=net, u_without_offset=True))]


def _over(mutant):
    """error / limit of the mutated fp64 chain's final bins on DENSE at F = 8."""
    _, _, params, ocfg, rays = po.state(DENSE)
    r64, r32 = po.references(DENSE)
    q0 = po.oracle_outputs(DENSE)["_debug"]["prop_q_0"]
    got = po.chain(params, ocfg, rays, q0, torch.float64, mutant=mutant)
    ok, e, _, limit = po.gate(got["ebins"], r64["ebins"], r32["ebins"])
    return ok, e / limit, got


def test_the_clean_chain_passes_its_own_gate():
    r64, r32 = po.references(DENSE)
    ok, e, e_ref, limit = po.gate(r64["ebins"], r64["ebins"], r32["ebins"])
    assert ok and e == 0.0 and limit > po.GATE_FACTOR * e_ref > 0
    ok2, e2, _, limit2 = po.gate(r32["ebins"], r64["ebins"], r32["ebins"], 2)     # the fp32 oracle passes at the project's 2
    assert ok2 and e2 <= limit2


@pytest.mark.parametrize("net", [0, 1])
def test_mutants_move_the_final_bins(net):
    mutants = list(itertools.chain.from_iterable(_level_mutants(net, level) for level in range(5))) + _net_mutants(net)
    failed = []
    for name, m in mutants:
        ok, ratio, _ = _over(m)
        print(f"DENSE, {name}: {ratio:.1f} x the limit at F = {po.GATE_FACTOR}")
        if ok:
            failed.append((name, ratio))
    assert not failed, failed


@pytest.mark.parametrize("net", [0, 1])
def test_the_one_mutant_no_output_can_see(net):
    """+ padding / N dropped: padding is exactly 0 on every ray at histogram_padding = 0.01 (the module docstring), so the bins, the medians
    and the positions are the clean chain's, every bit.  Reported, not dropped; asserted so that a config which makes it visible shows up."""
    ok, ratio, got = _over(po.Mutant(net=net, drop_padding_term=True))
    r64, _ = po.references(DENSE)
    print(f"DENSE, net {net}: + padding / N dropped: {ratio:.1f} x the limit -- NOT visible: 16 x 0.01 >= 1e-5, padding == 0 on every ray")
    assert ok and ratio == 0.0 and torch.equal(got["ebins"], r64["ebins"])
    for k in range(2):
        s = (r64["levels"][k]["weights"] + 0.01).sum(-1)
        assert float(s.min()) > 1e-5


def test_the_padding_term_is_seen_at_zero_histogram_padding():
    """The output that does see it: PDFSampler at histogram_padding = 0 on rays without weight, which tests/test_gpu_proposal_samples.py
    asks of ops.pdf_sample (the stage kernel shares SnPdfNorm with the proposal kernel)."""
    sbins, w = po.padding_case()
    r64, r32 = (po.resample(sbins, w, 8, 0.0, dt) for dt in (torch.float64, torch.float32))
    got = po.resample(sbins, w, 8, 0.0, torch.float64, po.Mutant(drop_padding_term=True))
    ok, e, _, limit = po.gate(got, r64, r32)
    print(f"histogram_padding = 0, a fifth of the rays without weight: + padding / N dropped: {e / limit:.0f} x the limit at F = {po.GATE_FACTOR}")
    assert not ok and e / limit > 100
    dead = w.sum(-1) == 0
    assert bool(dead.any()) and torch.equal(got[~dead], r64[~dead])
    assert bool((r64[dead][:, 1:] > r64[dead][:, :-1]).all())                       # a uniform pdf: resampled across the whole ray
    assert bool((got[dead] == sbins[dead, -1:].double()).all())                     # without the term: pdf 0, every bin on the last edge


def test_level_0_mutants_move_level_1_positions():
    """What part B of the GPU tests (prop_q_1) sees of net 0 without net 1 behind it."""
    _, _, params, ocfg, rays = po.state(DENSE)
    r64, r32 = po.references(DENSE)
    for name, m in _level_mutants(0, 2) + _net_mutants(0):
        _, _, got = _over(m)
        ok, e, _, limit = po.gate(got["levels"][1]["q"], r64["levels"][1]["q"], r32["levels"][1]["q"])
        print(f"DENSE, {name}: prop_q_1 {e / limit:.1f} x the limit")
        assert not ok, name


# ---- 4: the information condition -----------------------------------------------------------------------------------------------------------------
def test_medians_are_decided_and_weights_outweigh_the_padding():
    r64, r32 = po.references(DENSE)
    for k in range(2):
        cum64, cum32 = r64["levels"][k]["cumsum"], r32["levels"][k]["cumsum"]
        tie, margin = po.near_tie(cum32, cum64)
        share = float(tie.double().mean())
        quanta = float((cum64 - 0.5).abs().min()) / 2.0**-24
        print(f"DENSE level {k}: margin {margin:.2e}, rays within it of 0.5: {100 * share:.2f} %; nearest pass {quanta:.0f} quanta of 2^-24; "
              f"least cumulative weight {float(cum64[:, -1].min()):.3f}")
        assert share <= no.MAX_EXCLUDED
        assert float(cum64[:, -1].min()) > 0.5            # every ray's cumulative weight crosses 0.5: the median is a transmittance test
    t64, _ = po.references(po.case(setting="TWO"))
    _, _, _, ocfg, _ = po.state(po.case(setting="TWO"))
    for k in range(2):
        med = float(t64["levels"][k]["weights"].median())
        print(f"TWO level {k}: median proposal weight {med:.4f} against histogram_padding {ocfg.histogram_padding}")
        assert med > ocfg.histogram_padding


# ---- 5: where the GPU tests read the bins -----------------------------------------------------------------------------------------------------------
def test_final_bins_layout_is_the_frame_plan_of_the_gpu_tests_frames(tmp_path):
    """ops.final_bins_layout against sn_plan_frame (signerf_amd/csrc/sn_frame.h) through tests/c/frame_plan.cpp, built from that header
    alone: the 49 x 85 frame (8 x 8 tiles) and the 1 x 4165 frame (64 x 1 tiles), S = 16 behind two proposal levels and S = 32 behind one."""
    from signerf_amd import ops

    exe = str(tmp_path / "frame_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "c", "frame_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    chunk = po.config().eval_num_rays_per_chunk
    frames = [(h, w, S, nprop) for h, w in (no.FRAME, (1, no.N_RAYS)) for S, nprop in ((16, 2), (32, 1))]
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{h} {w} {S} {nprop} {chunk} 256 0 0\n" for h, w, S, nprop in frames))
    r = subprocess.run([exe, "table", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(frames)
    for (h, w, S, nprop), line in zip(frames, lines):
        f = dict(word.split("=", 1) for word in line.split())
        lay = ops.final_bins_layout(h, w, S, chunk)
        twl, thl, tx, ty = map(int, f["tiles"].split(","))
        assert (1 << twl, 1 << thl, tx, ty) == (lay["tile_w"], lay["tile_h"], lay["tiles_x"], lay["tiles_y"]), line
        assert (lay["tile_w"], lay["tile_h"]) == ((8, 8) if h >= 8 else (64, 1))
        assert int(f["main"].split(",")[2]) == lay["offset"] and int(f["prop"].split(",")[2]) == lay["offset"], line     # K1 reads where K2 wrote
        assert lay["floats"] == tx * ty * (S + 1) * 64 and lay["offset"] + 4 * lay["floats"] <= int(f["ws"])
