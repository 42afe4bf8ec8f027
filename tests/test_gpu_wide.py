"""Wide fields on the GPU: hidden_dim = hidden_dim_color = 128 (nerfstudio's nerfacto-big) through sn_wide_field_main_kernel and
sn_wide_field_stage_kernel (csrc/sn_wide_kernels.h), against the CPU oracle -- the field per sample, whole renders by every route, the
full-size table, the boundary of what a wide handle refuses, and one generator step.
Scenes: `BIG` on top of small_config, built with head_gain=6.0 (the default 3.0 gives a near-flat image at width 128: oracle rgb std
0.04-0.05; 6.0 gives 0.10-0.13); tiny-cuda-nn scenes are synthetic_tcnn_checkpoint's at average_init_density=3.0 as they are."""
import warnings

import pytest
import torch

from helpers import make_model, oracle_config, oracle_params_from_tcnn, rmse, small_config, synthetic_tcnn_checkpoint
from oracle import nerfacto as onf
from signerf_amd import Cameras, SceneBox, ops, scene
from signerf_amd._lib import SignerfHipError
from signerf_amd.datasetgenerator import DatasetGeneratorConfig, render_camera

pytestmark = pytest.mark.gpu
RMSE_TOL = 1e-3   # north_star's gate, as tests/test_gpu_render.py
BIG = dict(hidden_dim=128, hidden_dim_color=128, appearance_embed_dim=128, max_res=4096)
KEYS = ("rgb", "depth", "accumulation", "expected_depth")


def _wide(gpu, **kw):
    cfg = small_config(**{**BIG, **kw})
    model, sd = make_model(cfg, gpu, head_gain=6.0)
    return cfg, model, sd


def _wide_tcnn(gpu, **kw):
    kw.setdefault("average_init_density", 3.0)
    cfg = small_config(implementation="tcnn", **{**BIG, **kw})
    sd = synthetic_tcnn_checkpoint(cfg, seed=0)
    model = cfg.setup()
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    return cfg, model.to(gpu).eval(), sd


def _bundle(gpu, H, W, cam=0, focal=None, box=None):
    focal = focal or float(W)
    cams = Cameras(scene.benchmark_cameras(8)[:, :3], focal, focal, W / 2, H / 2, W, H).to(gpu)
    return cams[cam].generate_rays(camera_indices=0, aabb_box=box)


def _render(model, b):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # the "fp16x2 renders as fp32" notice of a wide handle (its own test below)
        return model.eval().get_outputs_for_camera_ray_bundle(b)


def _oracle(params, cfg, b):
    n = None if b.nears is None else b.nears.cpu()
    f = None if b.fars is None else b.fars.cpu()
    return onf.get_outputs_for_camera_ray_bundle(params, oracle_config(cfg), b.origins.cpu(), b.directions.cpu(), n, f)


def _gate(out, ref, keys):
    e = {k: rmse(out[k], ref[k]) for k in keys}
    print("wide render rmse", {k: f"{v:.2e}" for k, v in e.items()}, f"| oracle rgb std {float(ref['rgb'].std()):.3f} depth std {float(ref['depth'].std()):.3f}")
    for k in keys:
        assert out[k].shape == ref[k].shape and out[k].dtype == torch.float32 and out[k].is_cuda, k
    assert all(v <= RMSE_TOL for v in e.values()), e
    assert float(ref["rgb"].std()) > 0.05 and float(ref["depth"].std()) > 0.01   # non-vacuous


# ---- 1. the field, per sample ------------------------------------------------------------------------------------------------------
def _field_inputs():
    g = torch.Generator().manual_seed(5)
    n = 4165                                             # 65 waves + 5 lanes: more than one workgroup, a ragged last wave
    pos = (torch.rand(n, 3, generator=g) - 0.5) * 3.0
    pos[:100] *= 20.0                                    # far outside the unit box -> contraction branch
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    return pos, dirs


@pytest.mark.parametrize("app", [0, 32, 128])
@pytest.mark.parametrize("impl", ["torch", "tcnn"])
def test_wide_field_forward(gpu, impl, app):
    """ops.field_forward (sn_wide_field_stage_kernel: the same sn_wide_field_f32 the render kernel calls) against the oracle's field.
    Bounds: the 64-wide tests' own (tests/test_gpu_stages.py, tests/test_gpu_tcnn.py)."""
    if impl == "torch":
        cfg, model, params = _wide(gpu, appearance_embed_dim=app, num_proposal_iterations=0)
        dens_tol = 1e-4
    else:
        cfg, model, sd = _wide_tcnn(gpu, appearance_embed_dim=app, num_proposal_iterations=0)
        params = oracle_params_from_tcnn(sd, cfg)
        dens_tol = 2e-4
    ocfg = oracle_config(cfg)
    pos, dirs = _field_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        density, rgb, geo = ops.field_forward(model, pos.to(gpu), dirs.to(gpu), return_geo=True)
    rd, rh, _, _ = onf.density_field(params, "field.mlp_base", ocfg.main, pos[:, None, :], ocfg.average_init_density)
    rrgb = onf.field_rgb(params, ocfg, dirs, rh)[:, 0]
    rel = float(((density.cpu() - rd[:, 0, 0]).abs() / rd[:, 0, 0].clamp_min(1e-6)).max())
    e_rgb = float((rgb.cpu() - rrgb).abs().max())
    rgeo = rh[:, 0, 1:16]
    e_geo = float((geo.cpu() - rgeo).abs().max() / rgeo.abs().max())
    print(f"wide field [{impl}, app {app}]: density rel {rel:.2e}, rgb abs {e_rgb:.2e}, geo abs/max {e_geo:.2e}, oracle rgb std {float(rrgb.std()):.3f}")
    assert rel <= dens_tol
    assert e_rgb <= 2e-5
    assert e_geo <= 2e-5
    assert float(rrgb.std()) > 0.05


# ---- 2. render parity against the oracle on the same bundle ------------------------------------------------------------------------
def test_wide_render_uniform_64x64(gpu):
    cfg, model, sd = _wide(gpu, num_proposal_iterations=0, num_nerf_samples_per_ray=32)
    b = _bundle(gpu, 64, 64, cam=0)
    _gate(_render(model, b), _oracle(sd, cfg, b), KEYS)


def test_wide_render_proposals_ragged_45x59(gpu):
    cfg, model, sd = _wide(gpu, num_proposal_iterations=2, num_proposal_samples_per_ray=(48, 24), num_nerf_samples_per_ray=16)
    b = _bundle(gpu, 45, 59, cam=2, focal=70.0)
    _gate(_render(model, b), _oracle(sd, cfg, b), KEYS + ("prop_depth_0", "prop_depth_1"))


def test_wide_render_nerfacto_big_sample_counts_24x40(gpu):
    """(256, 128) proposal samples + 128 main samples: the most the proposal kernel takes (INTEGRATION.md "nerfacto-big")."""
    cfg, model, sd = _wide(gpu, log2_hashmap_size=14, num_proposal_iterations=2, num_proposal_samples_per_ray=(256, 128), num_nerf_samples_per_ray=128)
    b = _bundle(gpu, 24, 40, cam=3, focal=50.0)
    _gate(_render(model, b), _oracle(sd, cfg, b), KEYS + ("prop_depth_0", "prop_depth_1"))


@pytest.mark.parametrize("props", [0, 2])
def test_wide_render_tcnn_grid_40x56(gpu, props):
    cfg, model, sd = _wide_tcnn(gpu, num_proposal_iterations=props, num_proposal_samples_per_ray=(48, 24) if props else (), num_nerf_samples_per_ray=16)
    b = _bundle(gpu, 40, 56, cam=2, focal=60.0)
    _gate(_render(model, b), _oracle(oracle_params_from_tcnn(sd, cfg), cfg, b), KEYS + tuple(f"prop_depth_{i}" for i in range(props)))


def test_wide_render_aabb_nears_fars_with_misses(gpu):
    """As test_ragged_image_and_aabb_nears_fars: per-ray nears / fars from render_aabb; rays that miss carry the 1e10 sentinel."""
    cfg, model, sd = _wide(gpu, num_proposal_iterations=0, num_nerf_samples_per_ray=40)
    box = SceneBox(aabb=torch.tensor([[-0.15, -0.12, -0.1], [0.12, 0.15, 0.1]]))
    model.render_aabb = box
    b = _bundle(gpu, 45, 59, cam=2, focal=70.0, box=box)
    out, ref = _render(model, b), _oracle(sd, cfg, b)
    model.render_aabb = None
    hit = ref["depth"] < 1e6
    assert 0.05 < float(hit.float().mean()) < 1.0
    hg = hit.to(gpu)
    for k, c in (("rgb", 3), ("accumulation", 1), ("depth", 1), ("expected_depth", 1)):
        assert rmse(out[k][hg.expand(-1, -1, c)], ref[k][hit.expand(-1, -1, c)]) <= RMSE_TOL, k
    assert float(ref["rgb"][hit.expand(-1, -1, 3)].std()) > 0.05 and float(ref["depth"][hit].std()) > 0.01
    miss = ~hit
    assert float(out["accumulation"].cpu()[miss].abs().max()) == 0 and float(ref["accumulation"][miss].abs().max()) == 0
    assert torch.equal(torch.nan_to_num(out["rgb"].cpu()[miss.expand(-1, -1, 3)]), torch.nan_to_num(ref["rgb"][miss.expand(-1, -1, 3)]))
    assert torch.equal(torch.nan_to_num(out["depth"].cpu()[miss], nan=-1.0), torch.nan_to_num(ref["depth"][miss], nan=-1.0))


@pytest.mark.parametrize("option", [dict(proposal_initial_sampler="uniform"), dict(disable_scene_contraction=True)])
def test_wide_render_other_sampler_and_position_map_32x32(gpu, option):
    cfg, model, sd = _wide(gpu, num_proposal_iterations=2, num_proposal_samples_per_ray=(48, 24), num_nerf_samples_per_ray=16, **option)
    b = _bundle(gpu, 32, 32, cam=1, focal=40.0)
    _gate(_render(model, b), _oracle(sd, cfg, b), KEYS + ("prop_depth_0", "prop_depth_1"))


# ---- 3. the same answer by every route ---------------------------------------------------------------------------------------------
def test_wide_flat_bundle_equals_image_path(gpu):
    cfg, model, sd = _wide(gpu, num_proposal_iterations=0, num_nerf_samples_per_ray=24)
    b = _bundle(gpu, 32, 32, cam=4, focal=40.0)
    img = _render(model, b)
    flat = model.get_outputs(b.flatten())
    assert flat["rgb"].shape == (1024, 3)
    # (expected_depth too: 1024 rays are ONE chunk of the clip bounds on either path -- eval_num_rays_per_chunk is 32 768)
    for k, c in (("rgb", 3), ("depth", 1), ("accumulation", 1), ("expected_depth", 1)):
        assert torch.equal(flat[k].view(32, 32, c), img[k]), k


def test_wide_render_is_deterministic_256x256(gpu):
    """Two renders are bit-identical (an MFMA / permlane hazard slip shows as a few differing lanes per frame)."""
    cfg, model, sd = _wide(gpu, num_proposal_iterations=0, num_nerf_samples_per_ray=32)
    b = _bundle(gpu, 256, 256, cam=5)
    first, again = _render(model, b), _render(model, b)
    for k in KEYS:
        assert torch.equal(first[k], again[k]), k
    assert float(first["rgb"].std()) > 0.05


def test_wide_fp16x2_request_renders_exact_fp32_and_says_so(gpu):
    outs = {}
    for precision in ("fp16x2", "fp32"):
        cfg, model, sd = _wide(gpu, num_proposal_iterations=0, num_nerf_samples_per_ray=24, precision=precision)
        b = _bundle(gpu, 32, 32, cam=1, focal=40.0)
        if precision == "fp16x2":
            with pytest.warns(RuntimeWarning, match="fp32"):
                outs[precision] = model.eval().get_outputs_for_camera_ray_bundle(b)
        else:
            outs[precision] = model.eval().get_outputs_for_camera_ray_bundle(b)
        assert model.effective_precision == "fp32"
    for k in KEYS:
        assert torch.equal(outs["fp16x2"][k], outs["fp32"][k]), k


# ---- 4. the full-size table, once ----------------------------------------------------------------------------------------------------
def test_wide_full_size_table_2_to_21(gpu):
    """nerfacto-big's table (log2_hashmap_size 21, max_res 4096): 32-bit row arithmetic at 16 << 21 rows."""
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < (2 << 30):
        pytest.skip(f"needs 2 GB of free device memory, {free >> 20} MB free")
    cfg, model, sd = _wide(gpu, log2_hashmap_size=21, num_proposal_iterations=0, num_nerf_samples_per_ray=16)
    b = _bundle(gpu, 32, 48, cam=0, focal=48.0)
    _gate(_render(model, b), _oracle(sd, cfg, b), KEYS)
    assert ops.debug_layout(model)["n_dense"] == 0 and ops.debug_layout(model)["dense_bytes"] == 0   # a wide handle keeps no de-hashed copies


# ---- 5. the boundary -------------------------------------------------------------------------------------------------------------------
def test_wide_boundary_of_supported_shapes_and_calls(gpu):
    b = _bundle(gpu, 16, 16, cam=0, focal=20.0)
    # a default-width model before anything wide has run in this process
    dcfg = small_config(num_proposal_iterations=0, num_nerf_samples_per_ray=16)
    before = make_model(dcfg, gpu)[0].eval().get_outputs_for_camera_ray_bundle(b)
    before = {k: before[k].clone() for k in KEYS}

    for bad in (dict(hidden_dim=32), dict(hidden_dim=128, hidden_dim_color=64)):
        with pytest.raises(SignerfHipError, match=r"\(64, 64\) and \(128, 128\)"):
            small_config(num_proposal_iterations=0, **bad).setup().to(gpu).get_outputs_for_camera_ray_bundle(b)

    cfg, model, sd = _wide(gpu, num_proposal_iterations=0, num_nerf_samples_per_ray=16)
    good = _render(model, b)
    with pytest.raises(SignerfHipError, match="wide"):
        ops.render_rays_debug(model, b)
    with pytest.raises(SignerfHipError, match="wide"):
        ops.render_with_march_stats(model, b)
    with pytest.raises(SignerfHipError, match="wide"):
        good["normals"]
    again = _render(model, b)                                                 # the handle still renders after the refusals
    for k in KEYS:
        assert torch.equal(good[k], again[k]), k

    tcfg, tmodel, _ = _wide_tcnn(gpu, num_proposal_iterations=0, num_nerf_samples_per_ray=16, precision="fp16")
    with pytest.raises(SignerfHipError, match="wide"):
        _render(tmodel, b)
    tmodel.config.precision = "fp32"
    assert torch.isfinite(_render(tmodel, b)["rgb"]).all()

    with pytest.raises(NotImplementedError, match="wide"):
        small_config(**BIG, compute_normals="always").setup()

    # ... and a default-width model built afterwards renders what the one before did: the handles share no state
    after = make_model(dcfg, gpu)[0].eval().get_outputs_for_camera_ray_bundle(b)
    for k in KEYS:
        assert torch.equal(before[k], after[k]), k


# ---- 6. one generator step --------------------------------------------------------------------------------------------------------------
def test_wide_generator_render_camera(gpu):
    cfg, model, sd = _wide(gpu, num_proposal_iterations=0, num_nerf_samples_per_ray=32)
    cams = Cameras(scene.benchmark_cameras(8)[:, :3], 90.0, 90.0, 32.0, 32.0, 64, 64).to(gpu)
    gen = DatasetGeneratorConfig(aabb_min=[-0.25, -0.25, -0.25], aabb_max=[0.25, 0.25, 0.25], mask_dialation=(11, 11))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        rgb, mask, cond = render_camera(gen, model, cams[0])
    assert rgb.shape == (64, 64, 3) and mask.shape == (64, 64, 1) and cond.shape == (64, 64, 1)
    own = _render(model, cams[0].generate_rays(0))["rgb"]
    assert torch.equal(rgb, own) and float(own.std()) > 0.05


# ---- 7. early termination, carried over from sn_render_main_kernel ----------------------------------------------------------------------
@pytest.mark.parametrize("props", [0, 2])
def test_wide_early_termination_is_bit_identical_on_an_opaque_scene(gpu, monkeypatch, props):
    kw = dict(num_proposal_iterations=props)
    kw.update(dict(num_proposal_samples_per_ray=(64, 32), num_nerf_samples_per_ray=24) if props else dict(num_nerf_samples_per_ray=48))
    cfg = small_config(**{**BIG, **kw})
    model, _ = make_model(cfg, gpu, head_gain=6.0, density_bias=14.0)
    b = _bundle(gpu, 40, 56, cam=3, focal=60.0)
    out = {}
    for et in ("0", "1"):
        monkeypatch.setenv("SN_EARLY_TERM", et)
        ops.reload_env(model)
        o = _render(model, b)
        out[et] = {k: o[k].clone() for k in KEYS + tuple(f"prop_depth_{i}" for i in range(props))}
    monkeypatch.delenv("SN_EARLY_TERM")
    ops.reload_env(model)
    for k in out["0"]:
        assert torch.equal(out["0"][k].nan_to_num(-7.0), out["1"][k].nan_to_num(-7.0)), k
        assert torch.equal(torch.isnan(out["0"][k]), torch.isnan(out["1"][k])), k
    assert float(out["0"]["accumulation"].mean()) > 0.9     # the medium is dense: the termination had work to skip
