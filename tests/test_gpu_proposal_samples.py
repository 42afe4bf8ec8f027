"""The proposal kernel (csrc/sn_proposal.h sn_proposal_kernel) per SAMPLE and per hash LEVEL against the fp64 chain of
tests/proposal_oracle.py.

Every other value test of this kernel runs a stage kernel with other arithmetic (ops.field_forward, ops.pdf_sample) or is an image gate in
which one proposal level is a fifth of one net's signal.  Here the observable is what a PRODUCTION launch leaves for the main kernel: the
final euclidean bins (ops.render_with_final_bins), a continuous function of every proposal weight, so no ray and no bin is excluded; beside
them prop_depth_k and, where the instrumented launch exists (torch grid, two nets, default sampler and copies), the dumped prop_q_k.  The 4165
rays of normals_oracle.sample_set go in as a 49 x 85 frame (8 x 8 tiles, ragged on both edges) with per-ray nears / fars.

The chain starts at the kernel's own level-0 positions: ops.sample_positions at the oracle's level-0 euclidean bins, "fast" for the default
sampler (the instrumented launch's prop_q_0 must be that q0, every bit) and "strict" for the uniform-sampler (ALT) instantiation (which
must be the oracle's prop_q_0, every bit).  That entry point has no box map, so the box (ALT) cases start at the oracle's prop_q_0 (_q0).

A. the whole chain, every instantiation: <0,5,4>, <0,-1,-1,ALT> (box; uniform sampler), <1,5,4>, <1,-1,-1,ALT>, <1,-1,-1> (a grid whose
   5 + 5 levels are all dense), <0,-1,-1> and <1,-1,-1> behind ONE net -- on TWO and DENSE (proposal_oracle.SETTINGS);
B. level 0 alone: the dumped prop_q_1 against the chain's;
C. one or two levels of one net kept, the rest of its table zeroed (DENSE): net 0's coefficient copies (levels 0-3 register-cached, 4
   re-fetched), net 1's copies and its copy | x-paired-table boundary (3,4), the same boundaries with no copies at all, the tiny-cuda-nn
   dense | hashed boundary;
D. tables x 1e-3 (nerfstudio's magnitudes: the fp16 hi+lo operands' conditioning);
E. the medians: prop_depth_0 bit for bit, prop_depth_1 under the gate, on the rays whose cumsum does not pass 0.5 within rounding;
F. lane independence: the same rays as a 1 x 4165 frame (64 x 1 tiles) and next to rays with a NaN origin (every third ray; lanes 32-63 of
   every other tile -- the MFMA tile that lanes j and j + 32 share): the healthy rays' bits do not move, the NaN rays are resampled
   uniformly as the oracle does.  Handled values: nothing here is meant to fault;
G. SnPdfNorm's "+ padding / N", which is exactly 0 in every render, through ops.pdf_sample at histogram_padding = 0.

Gate (proposal_oracle.gate): max |kernel - ref64| <= F x max |ref32 - ref64| + 1 ulp of the largest output.  F: see FACTOR below and
DESIGN.md K2, which holds the measured table.  tests/test_proposal_oracle_host.py shows that every single wrong term exceeds the limit at
F = 8.  Every case prints its figures before it asserts."""
import pytest
import torch

import normals_oracle as no
import proposal_oracle as po
from oracle import tcnn_layout as tl
from signerf_amd import RayBundle, ops

pytestmark = pytest.mark.gpu
_MODELS = {}
# The project's gate has factor 2 (hashgrid_oracle.gate); every output starts there and, measured (DESIGN.md K2 holds the table), every
# output stays there -- the final bins of every torch-grid, ALT, one-net and all-dense case <= 1.47, prop_q_1 <= 1.02, prop_depth_1 0.89 --
# but one: the final bins behind TWO levels of the tiny-cuda-nn grid's bias-free nets in <1,5,4> ("bins-tcnn": 0.85-2.29, the one above 2
# being the whole chain on TWO).  The split-precision MLP is not it (the fp64 chain with fp16 hi + lo operands moves the bins by 1-3 % of
# e_ref32).  e_ref32 there is the rounding of the level-1 POSITIONS (q1 alone rounded to fp32, everything else fp64: 4.9e-6 of its 7.7e-6;
# level 4 of net 1 multiplies an ulp of q by 255 and bias-free nets swing exp(h0) over e^+-3 along a ray), both errors are maxima over
# 4165 x 17 bins that one ill-conditioned ray decides, and the kernel's q1 (sn_sample_q_fast: fma position, v_rcp_f32 contraction) is
# another rounding of the same position than the oracle's: the two distributions agree to two digits up to the 99.9th percentile
# (3.5e-6 / 3.5e-6) and the kernel's maximum sits on the ray that +-0.5 and +-2 ulp of noise on q1 in the fp64 chain also single out
# (ray 437: 5.3e-6 and 2.4e-5; kernel 1.76e-5; fp32 chain there 2.0e-6).  For that output alone normals_oracle.GATE_FACTOR = 8 applies; a
# ratio beyond 8 is a finding, not a tolerance to widen.
FACTOR = {"bins-tcnn": po.GATE_FACTOR}


def _bins_output(c):
    """Which FACTOR entry a case's final bins fall under: two levels of small_config's tiny-cuda-nn nets behind the fast position map
    (<1,5,4>), or everything else -- the ALT instantiations' strict map (measured 1.00-1.13), one net, the all-dense nets."""
    return "bins-tcnn" if c[:3] == ("tcnn", "contract", "piecewise") and c[3] != "ONE" and c[6] is None else "bins"


def _factor(output):
    return FACTOR.get(output, 2)


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(gpu):
    """A device error ends the session: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize(gpu)
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _model(gpu, c, dense_levels=0):
    """One model per configuration, re-used across cases by loading the case's state dict."""
    impl, kind, sampler, setting, _, _, nets = c
    cfg, sd, _, _, rays = po.state(c)
    key = (impl, kind, sampler, setting, nets, dense_levels, str(gpu))
    if key not in _MODELS:
        _MODELS[key] = po.config(impl, kind, sampler, setting, nets, dense_levels=dense_levels).setup().to(gpu).eval()
    model = _MODELS[key]
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    return model, rays


def _bundle(rays, gpu, shape, origins=None):
    t = {k: rays[k].to(gpu) for k in ("o", "d", "near", "far")}
    if origins is not None:
        t["o"] = origins.to(gpu)
    t = {k: v.view(*shape, v.shape[-1]) for k, v in t.items()}
    return RayBundle(origins=t["o"], directions=t["d"], pixel_area=torch.ones_like(t["near"]), nears=t["near"], fars=t["far"])


def _selected(model, c):
    """sn_select_proposal (csrc/sn_variant.h) from what the handle holds: (GRID, ND0, ND1, ALT)."""
    impl, kind, sampler = c[:3]
    cfg = model.config
    n = cfg.num_proposal_iterations
    nd = [ops.debug_layout(model, k)["n_dense"] for k in range(n)]
    tcnn, alt = int(impl == "tcnn"), kind == "box" or sampler != "piecewise"
    default = n == 2 and nd == [5, 4]
    if alt:
        return (tcnn, -1, -1, True)
    if tcnn:
        args = cfg.proposal_net_args_list
        td = [sum(tl.grid_meta(a["num_levels"], a.get("base_res", 16), a["max_res"], a["log2_hashmap_size"]).dense) for a in args[:n]]
        return (1, 5, 4, False) if default and td[0] <= 5 and td[1] <= 4 else (1, -1, -1, False)
    return (0, 5, 4, False) if default else (0, -1, -1, False)


def _q0(gpu, c, rays, origins=None):
    """The kernel's own level-0 positions [R, N0, 3] at the oracle's level-0 bins.  ops.sample_positions runs the three position maps under the
    scene contraction only (its entry point takes no SnPosMap), so the box instantiations start at the oracle's own prop_q_0: their strict map
    (csrc/sn_device.h sn_sample_q) shares the position step that the uniform-sampler case holds to the oracle bit for bit and then forms
    (p - lo) / len with the oracle's operations in its order, contraction off."""
    if c[1] == "box":
        assert origins is None
        return po.oracle_outputs(c)["_debug"]["prop_q_0"]
    eb = po.level0_bins(c)
    n0 = eb.shape[1] - 1
    o = (rays["o"] if origins is None else origins)[:, None, :].expand(-1, n0, -1).reshape(-1, 3)
    d = rays["d"][:, None, :].expand(-1, n0, -1).reshape(-1, 3)
    alt = c[1] == "box" or c[2] != "piecewise"
    got = ops.sample_positions(o.to(gpu), d.to(gpu), eb[:, :-1].reshape(-1).to(gpu), eb[:, 1:].reshape(-1).to(gpu))
    return got["strict" if alt else "fast"].view(-1, n0, 3).cpu()


def _render(gpu, c, dense_levels=0, shape=no.FRAME, origins=None, want=None):
    """The production launch -> dict(bins [R,S+1], prop_depth_k [R,1], q0, model, rays), everything on the CPU; asserts the instantiation,
    and where the instrumented launch exists that it equals the production one bit for bit (dump: its tensors)."""
    model, rays = _model(gpu, c, dense_levels)
    bundle = _bundle(rays, gpu, shape, origins)
    prod, bins = ops.render_with_final_bins(model, bundle)
    again = model.get_outputs_for_camera_ray_bundle(bundle)
    n = model.config.num_proposal_iterations
    for k in ("rgb", "depth", "accumulation", "expected_depth"):
        assert torch.equal(prod[k].view(torch.int32), again[k].view(torch.int32)), k
    out = {"bins": bins.cpu(), "q0": _q0(gpu, c, rays, origins), "rays": rays, "selected": _selected(model, c)}
    out.update({f"prop_depth_{k}": again[f"prop_depth_{k}"].reshape(no.N_RAYS, 1).cpu() for k in range(n)})
    if want is not None:
        assert out["selected"] == want, f"{po.case_id(c)}: {out['selected']} ran, {want} was meant"
    if out["selected"] == (0, 5, 4, False):
        dbg_out, dump = ops.render_rays_debug(model, bundle, want=("prop_q", "pdf_index", "final_bins"))
        for k in ("rgb", "depth", "accumulation", "expected_depth"):
            assert torch.equal(dbg_out[k].view(torch.int32), prod[k].view(torch.int32)), f"{k}: the instrumented kernels differ from the production ones"
        assert torch.equal(dump["final_bins"].view(torch.int32), bins.view(torch.int32)), "the instrumented launch's bins are not the production launch's"
        q0_dump = dump["prop_q_0"].view(no.N_RAYS, -1, 3).cpu()
        live = torch.ones(no.N_RAYS, dtype=torch.bool) if origins is None else torch.isfinite(origins).all(-1)
        assert torch.equal(q0_dump[live].view(torch.int32), out["q0"][live].view(torch.int32)), "the dumped prop_q_0 is not the position map at the oracle's level-0 bins"
        assert bool(torch.isnan(q0_dump[~live]).any(-1).all()) and bool(torch.isnan(out["q0"][~live]).any(-1).all())
        out["dump"] = {k: v.cpu() for k, v in dump.items()}
    if out["selected"][3]:
        want_q0 = po.oracle_outputs(c)["_debug"]["prop_q_0"]
        if origins is None:
            assert torch.equal(out["q0"].view(torch.int32), want_q0.view(torch.int32)), "the strict position map is not the oracle's prop_q_0"
    return out


def _sound(name, bins, rays):
    assert bins.shape[0] == no.N_RAYS and bins.dtype == torch.float32 and bool(torch.isfinite(bins).all()), name
    assert bool((bins[:, 1:] > bins[:, :-1]).all()), f"{name}: bins not strictly increasing"
    assert bool((bins[:, 0] >= rays["near"][:, 0] * (1 - 1e-6)).all()) and bool((bins[:, -1] <= rays["far"][:, 0] * (1 + 1e-6)).all()), name


def _gate(name, output, got, ref64, ref32, rows=slice(None)):
    factor = _factor(output)
    ok, e, e_ref, limit = no.gate(got.reshape(got.shape[0], -1), ref64.reshape(got.shape[0], -1), ref32.reshape(got.shape[0], -1), rows, factor)
    print(f"{name}: {output}: e_hip {e:.2e} e_ref32 {e_ref:.2e} F {factor} limit {limit:.2e} ratio {e / e_ref:.2f}")
    return ok, f"{name}: {output}: {e:.3e} > {limit:.3e}"


def _check_chain(name, r, c):
    """Part A's check: the final bins of the production launch against the chain at the kernel's own q0."""
    _sound(name, r["bins"], r["rays"])
    r64, r32 = po.references(c, r["q0"])
    ok, msg = _gate(name, _bins_output(c), r["bins"], r64["ebins"], r32["ebins"])
    assert ok, msg
    return r64, r32


def _name(c, dense_levels=0):
    return po.case_id(c) + (f" dense_levels={dense_levels}" if dense_levels else "")


# ---- A: the whole chain, every instantiation ---------------------------------------------------------------------------------------------------
WHOLE = [("torch", "contract", "piecewise", None, (0, 5, 4, False)), ("torch", "box", "piecewise", None, (0, -1, -1, True)),
         ("torch", "contract", "uniform", None, (0, -1, -1, True)), ("tcnn", "contract", "piecewise", None, (1, 5, 4, False)),
         ("tcnn", "box", "piecewise", None, (1, -1, -1, True)), ("tcnn", "contract", "piecewise", "all-dense", (1, -1, -1, False))]


@pytest.mark.parametrize("setting", ["TWO", "DENSE"])
@pytest.mark.parametrize("impl,kind,sampler,nets,want", WHOLE, ids=lambda v: None if isinstance(v, tuple) else str(v))
def test_whole_chain(gpu, impl, kind, sampler, nets, want, setting):
    c = po.case(impl, kind, sampler, setting, nets=nets)
    r = _render(gpu, c, want=want)
    _check_chain(f"{_name(c)} <{want}>", r, c)


@pytest.mark.parametrize("impl,want", [("torch", (0, -1, -1, False)), ("tcnn", (1, -1, -1, False))])
def test_whole_chain_behind_one_net(gpu, impl, want):
    """One proposal level of 16 samples, 32 main samples: the run-time variants, every level from the x-paired / the uploaded tables."""
    c = po.case(impl, setting="ONE")
    r = _render(gpu, c, want=want)
    _check_chain(f"{_name(c)} <{want}>", r, c)


# ---- B: level 0 alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["TWO", "DENSE"])
def test_level_0_through_the_positions_of_level_1(gpu, setting):
    """Net 0, the first resampling step, the spacing map and the position map, without net 1 behind them."""
    c = po.case(setting=setting)
    r = _render(gpu, c, want=(0, 5, 4, False))
    r64, r32 = po.references(c, r["q0"])
    q1 = r["dump"]["prop_q_1"].view(no.N_RAYS, -1, 3)
    assert bool(torch.isfinite(q1).all()) and float(q1.min()) >= 0 and float(q1.max()) < 1
    ok, msg = _gate(_name(c), "prop_q_1", q1, r64["levels"][1]["q"], r32["levels"][1]["q"])
    assert ok, msg


# ---- C: per level -------------------------------------------------------------------------------------------------------------------------------
SINGLES_AND_PAIRS = [(k,) for k in range(5)] + [(k, k + 1) for k in range(4)]


def _levels_id(levels):
    return "L" + "+".join(str(k) for k in levels)


@pytest.mark.parametrize("levels", SINGLES_AND_PAIRS, ids=_levels_id)
@pytest.mark.parametrize("net", [0, 1])
def test_levels_of_one_net(gpu, net, levels):
    """Net 0: all coefficient copies, levels 0-3 kept in registers across the steps, level 4 re-fetched.  Net 1: copies 0-3, level 4 from the
    x-paired table -- (3,4) carries the feature scale across that boundary.  The other net stays whole."""
    c = po.case(setting="DENSE", keep=(net, levels))
    _check_chain(_name(c), _render(gpu, c, want=(0, 5, 4, False)), c)


@pytest.mark.parametrize("net,levels", [(0, (4,)), (1, (3,)), (1, (4,)), (1, (3, 4))], ids=lambda v: str(v) if isinstance(v, int) else _levels_id(v))
def test_boundary_levels_without_copies(gpu, net, levels):
    """The same boundaries with every level from the x-paired tables (no de-hashed copies: <0,-1,-1>)."""
    c = po.case(setting="DENSE", keep=(net, levels))
    _check_chain(_name(c, -1), _render(gpu, c, dense_levels=-1, want=(0, -1, -1, False)), c)


@pytest.mark.parametrize("levels", [(0,), (1,), (0, 1)], ids=_levels_id)
@pytest.mark.parametrize("net", [0, 1])
def test_tcnn_dense_hashed_boundary(gpu, net, levels):
    """T = 2^12: level 0 (16^3 rows) is indexed densely, level 1 through the hash."""
    c = po.case("tcnn", setting="DENSE", keep=(net, levels))
    cfg = po.state(c)[0]
    a = cfg.proposal_net_args_list[net]
    assert tl.grid_meta(a["num_levels"], a.get("base_res", 16), a["max_res"], a["log2_hashmap_size"]).dense[:2] == [True, False]
    _check_chain(_name(c), _render(gpu, c, want=(1, 5, 4, False)), c)


# ---- D: tables of realistic magnitude -------------------------------------------------------------------------------------------------------------
def test_tables_of_realistic_magnitude(gpu):
    """Both nets' tables x 1e-3 (nerfstudio's initialisation): the fp16 hi+lo operands at that magnitude.  A conditioning case: the gate
    must hold; no sensitivity is claimed (the densities are nearly constant)."""
    c = po.case(setting="DENSE", scale=1e-3)
    _check_chain(_name(c), _render(gpu, c, want=(0, 5, 4, False)), c)


# ---- E: the medians -------------------------------------------------------------------------------------------------------------------------------
def test_medians(gpu):
    c = po.case(setting="DENSE")
    r = _render(gpu, c, want=(0, 5, 4, False))
    r64, r32 = po.references(c, r["q0"])
    results = []
    for k in range(2):
        tie, margin = po.near_tie(r32["levels"][k]["cumsum"], r64["levels"][k]["cumsum"])
        share = float(tie.double().mean())
        print(f"{_name(c)}: level {k}: {100 * share:.2f} % of the rays pass 0.5 within {margin:.2e} and are left out")
        assert share <= no.MAX_EXCLUDED
        got, keep = r[f"prop_depth_{k}"], ~tie
        if k == 0:      # level 0's bins are the oracle's own: the mid-point of the reference's median bin, every bit
            same = got.view(torch.int32) == r32["levels"][0]["median"].view(torch.int32)
            print(f"{_name(c)}: prop_depth_0: {int((~same[keep]).sum())} of {int(keep.sum())} rays differ from the reference's mid-point")
            results.append((bool(same[keep].all()), "prop_depth_0 is not the reference's median mid-point"))
        else:
            results.append(_gate(_name(c), "prop_depth_1", got, r64["levels"][1]["median"], r32["levels"][1]["median"], keep))
    for ok, msg in results:
        assert ok, msg


# ---- F: lane independence -------------------------------------------------------------------------------------------------------------------------
def test_frame_shape(gpu):
    """The same rays as a 1 x 4165 frame (64 x 1 tiles: other lanes share a wave, a tile and the j | j + 32 MFMA tile): every ray's bits."""
    c = po.case(setting="TWO")
    frame = _render(gpu, c, want=(0, 5, 4, False))
    row = _render(gpu, c, shape=(1, no.N_RAYS), want=(0, 5, 4, False))
    for k in ("bins", "prop_depth_0", "prop_depth_1"):
        assert torch.equal(frame[k].view(torch.int32), row[k].view(torch.int32)), k


def _poison_patterns():
    i = torch.arange(no.N_RAYS)
    y, x = i // no.FRAME[1], i % no.FRAME[1]
    tile = (y // 8) * -(-no.FRAME[1] // 8) + x // 8
    return {"every third ray": i % 3 == 0, "lanes 32-63 of every other tile": (tile % 2 == 0) & (y % 8 >= 4)}


@pytest.mark.parametrize("pattern", list(_poison_patterns()))
def test_rays_next_to_nan_rays(gpu, pattern):
    """A NaN origin coordinate is NaN through the reference's whole field; nan_to_num makes the ray's weights 0 and it is resampled uniformly.
    The kernel's 32 x 32 MFMA tile serves lanes j and j + 32 together: the healthy rays' bins and medians must not move by a bit."""
    c = po.case(setting="TWO")
    dead = _poison_patterns()[pattern]
    clean = _render(gpu, c, want=(0, 5, 4, False))
    rays = clean["rays"]
    origins = torch.where(dead[:, None] & (torch.arange(3) == 1), torch.full((), float("nan")), rays["o"])
    bad = _render(gpu, c, origins=origins, want=(0, 5, 4, False))
    assert 0.2 < float(dead.double().mean()) < 0.4
    for k in ("bins", "prop_depth_0", "prop_depth_1"):
        assert torch.equal(bad[k][~dead].view(torch.int32), clean[k][~dead].view(torch.int32)), f"{k} of the healthy rays moved"
    _sound(pattern, bad["bins"], rays)
    _, _, params, ocfg, _ = po.state(c)
    r64 = po.chain(params, ocfg, rays, bad["q0"], torch.float64, dead=dead)
    r32 = po.chain(params, ocfg, rays, bad["q0"], torch.float32, dead=dead)
    assert float(r64["levels"][0]["weights"][dead].abs().max()) == 0 and float(r64["levels"][1]["weights"][dead].abs().max()) == 0
    results = [_gate(f"{_name(c)}, {pattern}, the NaN rays", "bins", bad["bins"][dead], r64["ebins"][dead], r32["ebins"][dead]),
               _gate(f"{_name(c)}, {pattern}, all rays", "bins", bad["bins"], r64["ebins"], r32["ebins"])]
    for ok, msg in results:
        assert ok, msg


# ---- G: the one term no render reaches ----------------------------------------------------------------------------------------------------------
def test_padding_term_of_the_pdf_norm(gpu):
    """SnPdfNorm's "+ padding / N" is exactly 0 in every render (a handle's histogram_padding is nerfacto's 0.01), so the final bins cannot see
    it (tests/test_proposal_oracle_host.py).  The stage kernel behind ops.pdf_sample shares SnPdfNorm with the proposal kernel: at
    histogram_padding = 0, rays without any weight are resampled uniformly through that term alone."""
    sbins, w = po.padding_case()
    got, _ = ops.pdf_sample(sbins.to(gpu), w.to(gpu), 8, histogram_padding=0.0)
    r64, r32 = (po.resample(sbins, w, 8, 0.0, dt) for dt in (torch.float64, torch.float32))
    dead = w.sum(-1) == 0
    results = [_gate("histogram_padding 0, rays without weight", "pdf_bins", got.cpu()[dead], r64[dead], r32[dead]),
               _gate("histogram_padding 0, all rays", "pdf_bins", got.cpu(), r64, r32)]
    for ok, msg in results:
        assert ok, msg
