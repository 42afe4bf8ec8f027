"""The render kernel (csrc/sn_main.h sn_render_main_kernel, csrc/sn_wide_kernels.h sn_wide_field_main_kernel) per SAMPLE: with
one main sample per ray ("num_nerf_samples_per_ray=1") and the "last_sample" background the rendered colour of a ray IS its sample's colour
(rgb = w c + (1 - w) c = c whatever w is) and its accumulation IS the sample's weight w = 1 - exp(-sigma delta), sigma =
average_init_density exp(h0) selector, delta = t1 - t0; a hash table with all but one or two levels zeroed puts those levels' read path alone in
front of both MLPs.

This module restates the six outputs of such a ray (c, w, rgb, accumulation, depth, expected_depth) in a given dtype from the fp32 inputs the
oracle itself works on -- the normalised positions q, the selector, the two bin edges and the ray direction: fp64 is the reference the gate
measures against, fp32 is "the oracle at a given q" (what is compared with oracle.nerfacto on the CPU, and e_ref32 behind the proposal sampler,
where the kernel's own q is the only q there is).  The density side is tests/normals_oracle.density_h (cells and in-voxel offsets decided in
fp32, blend and MLP in the dtype); the colour head (direction encoding, mean appearance embedding, field.mlp_head, sigmoid), the density
activation, the weight and the four renderers are restated here.  Single terms can be MUTATED: the host tests feed the mutants to the gate to
show that it can fail.  Unlike the normals these values are continuous across voxel faces and ReLU kinks: no sample is excluded."""
import dataclasses

import torch

import hashgrid_oracle as ho
import normals_oracle as no
from helpers import onf

OUTPUTS = ("rgb", "accumulation", "depth", "expected_depth")
PROPOSAL_SAMPLES = (8, 4)      # behind the proposal sampler: two proposal levels of this many samples, then the one main sample
BIG = dict(hidden_dim=128, hidden_dim_color=128, appearance_embed_dim=128, max_res=4096)     # tests/test_gpu_wide.py's wide config
WIDE_HEAD_GAIN = 6.0
WHITE = (1.0, 1.0, 1.0)
TAU_RANGE = (0.05, 5.0)        # sigma delta in here: w = 1 - exp(-tau) in [0.049, 0.993], |d w / d ln sigma| = tau exp(-tau) >= 0.034
MIN_INFORMATIVE = 0.9
# The project's gate has factor 2 (hashgrid_oracle.gate).  Measured on the hardware over every case of tests/test_gpu_render_samples.py
# (DESIGN.md K1 holds the table): every exact-fp32 case is at most 1.65; the 27 ratios above 2 are all fp16x2 -- rgb 2.0-5.3 (22-bit split
# operands through five layers), accumulation 5.0-6.4 (the density layer's accumulator starts at its bias, so its 12 MFMA steps round at the
# bias's size, and exp(h0) hands that to the weight) -- each the whole distribution's, not one sample's.  For those explained outputs, and for
# them alone (gate_factor), the factor the same split operands were measured at in the normals kernel applies (normals_oracle.GATE_FACTOR
# = 8); everything else is held to 2.  A ratio beyond 8 is a finding, not a tolerance to widen: the exact-fp32 density layer was one (8.1
# 64-wide, 11.5 wide) and now adds its bias last (csrc/sn_main.h).  gate()'s default is 8: the host tests' mutants must exceed even that.
GATE_FACTOR = no.GATE_FACTOR


def gate_factor(precision, output):
    """The factor a kernel output is held to: the project's 2, and GATE_FACTOR for the rgb and the accumulation of the split-precision
    arithmetic alone (the explained cases; depth and expected_depth have no MLP in them)."""
    return GATE_FACTOR if precision == "fp16x2" and output in ("rgb", "accumulation") else 2


@dataclasses.dataclass
class Mutant:
    """One wrong term of the render of a sample (None of them: the restatement itself)."""
    level: int = -1                  # the hash level the next four act on
    feature_factor: float = 1.0      # that level's blended features times this
    drop_cross_term: bool = False    # that level blended as A + ox B + oy C per z slice: the D of A + ox B + oy (C + ox D) dropped
    swap_corners: bool = False       # corners 1 <-> 3 exchanged at that level
    feat_scale: float = 1.0          # the power-of-two feature scale the other levels carry left off that level (its features / this)
    density_factor: float = 1.0      # sigma times this
    flip_sh: int = -1                # this component of the direction encoding negated
    shifted_geo: bool = False        # the colour head fed h[:, 0:15] instead of h[:, 1:16]
    appearance_row_0: bool = False   # row 0 of the appearance table instead of its mean

    @property
    def touches_grid(self):
        return self.level >= 0 and (self.feature_factor != 1.0 or self.drop_cross_term or self.swap_corners or self.feat_scale != 1.0)


# ---- the density side -------------------------------------------------------------------------------------------------------------------------
def coefficient_blend(f, o, cross=True):
    """hashgrid_oracle.blend in the form the de-hashed copies of the coarse levels hold: per z slice A + ox B + oy (C + ox D) with A the
    floor-floor corner, B / C the differences along x / y and D the mixed one (corner order: hashgrid_oracle.CORNERS, x y z)."""
    ox, oy, oz = o[..., 0:1], o[..., 1:2], o[..., 2:3]

    def plane(cc, cf, ff, fc):
        A, B, C, D = ff, cf - ff, fc - ff, cc - cf - fc + ff
        return A + ox * B + oy * (C + ox * D if cross else C)

    up, down = plane(f[0], f[1], f[2], f[3]), plane(f[4], f[5], f[6], f[7])
    return down + oz * (up - down)


def density_h(params, ocfg, q, dtype=torch.float64, mutant=None):
    """h [N,16]: normals_oracle.density_h's; with a mutant that touches the grid the same arithmetic with that level's features changed."""
    if mutant is None or not mutant.touches_grid:
        return no.density_h(params, ocfg, q, dtype)[0]
    grid = no.grid_of(params, ocfg)
    idx, off = no.cells(q, grid)
    f, o, k = ho.gather(grid["table"].to(dtype), idx), off.to(dtype), mutant.level
    if mutant.swap_corners:
        f = [v.clone() for v in f]
        f[1][:, k], f[3][:, k] = f[3][:, k].clone(), f[1][:, k].clone()
    enc = ho.blend(f, o).clone()
    if mutant.drop_cross_term:
        enc[:, k] = coefficient_blend([v[:, k] for v in f], o[:, k], cross=False)
    enc[:, k] *= mutant.feature_factor / mutant.feat_scale
    W0, b0, W1, b1 = no._mlp0(params, dtype)
    return torch.relu(enc.flatten(-2, -1) @ W0.T + b0) @ W1.T + b1


# ---- the colour head --------------------------------------------------------------------------------------------------------------------------
def colour(params, ocfg, d, h, dtype=torch.float64, mutant=None):
    """oracle.nerfacto.field_rgb for one sample per ray: d [N,3] fp32 ray directions, h [N,16] -> c [N,3] in dtype: direction encoding (both
    sh_remap forms), geometry features, the mean appearance embedding (eval mode) -> field.mlp_head -> sigmoid."""
    assert d.dtype == torch.float32
    enc = onf.direction_encoding(d.to(dtype), ocfg)
    if mutant is not None and mutant.flip_sh >= 0:
        enc = enc.clone()
        enc[:, mutant.flip_sh] *= -1
    geo = h[:, 0:ocfg.geo_feat_dim] if (mutant is not None and mutant.shifted_geo) else h[:, 1:1 + ocfg.geo_feat_dim]
    table = params["field.embedding_appearance.embedding.weight"].to(dtype)
    app = table[0] if (mutant is not None and mutant.appearance_row_0) else table.mean(dim=0)
    x = torch.cat([enc, geo.to(dtype), torch.ones((d.shape[0], app.numel()), dtype=dtype) * app], dim=-1)
    for i in range(3):
        x = torch.nn.functional.linear(x, params[f"field.mlp_head.layers.{i}.weight"].to(dtype), params[f"field.mlp_head.layers.{i}.bias"].to(dtype))
        if i < 2:
            x = torch.relu(x)
    return torch.sigmoid(x)


# ---- one sample per ray through the renderers ------------------------------------------------------------------------------------------------
def composite(c, sigma, t0, t1, background=None):
    """RaySamples.get_weights and the RGB / accumulation / median-depth / expected-depth renderers for ONE sample per ray, in c's dtype:
    c [N,3], sigma, t0, t1 [N,1]; background None: "last_sample", else a constant colour.  The transmittance in front of the only sample is
    exp(-0) = 1; the clip bounds of the expected depth are those of the whole set (one chunk)."""
    delta, mid = t1 - t0, (t0 + t1) / 2
    w = torch.nan_to_num((1 - onf._exp(-(delta * sigma))) * onf._exp(torch.zeros_like(sigma)))
    c = torch.nan_to_num(c)
    bg = c if background is None else torch.tensor(background, dtype=c.dtype).expand_as(c)
    rgb = torch.clamp(w * c + bg * (1.0 - w), min=0.0, max=1.0)
    expected = torch.clip((w * mid) / (w + 1e-10), mid.min(), mid.max())
    return {"c": c, "w": w, "tau": delta * sigma, "rgb": rgb, "accumulation": w, "depth": mid, "expected_depth": expected}


def sample(params, ocfg, q, selector, bins, d, dtype=torch.float64, background=None, mutant=None):
    """The render of N one-sample rays in dtype: q [N,3] fp32 (normalised, selector-multiplied), selector [N] bool, bins [N,2] fp32 (the
    euclidean edges of the one bin), d [N,3] fp32 -> dict(c, w, tau, rgb, accumulation, depth, expected_depth, h)."""
    assert q.dtype == torch.float32 and bins.dtype == torch.float32 and d.dtype == torch.float32
    h = density_h(params, ocfg, q, dtype, mutant)
    sigma = ocfg.average_init_density * torch.exp(h[:, 0:1]) * selector[:, None].to(dtype)
    if mutant is not None:
        sigma = sigma * mutant.density_factor
    out = composite(colour(params, ocfg, d, h, dtype, mutant), sigma, bins[:, 0:1].to(dtype), bins[:, 1:2].to(dtype), background)
    out["h"] = h
    return out


def gate(got, ref64, ref32, factor=GATE_FACTOR):
    """normals_oracle.gate over EVERY sample: e_hip = max |got - ref64| <= factor x e_ref32 + 1 ulp of the largest output, e_ref32 =
    max |ref32 - ref64| (the fp32 oracle's own error, never the kernel's) -> (ok, e_hip, e_ref32, the limit)."""
    return no.gate(got, ref64, ref32, slice(None), factor)


def informative(tau):
    """The share of samples whose accumulation says something about the density: sigma delta inside TAU_RANGE (from the reference alone)."""
    return float(((tau >= TAU_RANGE[0]) & (tau <= TAU_RANGE[1])).double().mean())


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
# (impl, levels, scale, kind, sampler) as normals_oracle.all_cases(), plus: wide (the 128-wide fields), proposals (behind the proposal sampler)
# and the background.  average_init_density of a tiny-cuda-nn case is normals_oracle.config's 3.0: every case meets the information condition
# with it (tests/test_render_oracle_host.py; the least share is 92 %, all levels on the tiny-cuda-nn grid).
_CASES = {}


def config(impl="torch", kind="contract", sampler="piecewise", wide=False, proposals=False, background="last_sample", **kw):
    """normals_oracle.config's model config (one main sample, per-ray nears / fars) with K1 alone: no normals; optionally wide, behind two
    proposal levels, with a constant background."""
    from helpers import small_config

    if impl == "tcnn":
        kw.setdefault("average_init_density", 3.0)
    if wide:
        kw = {**BIG, **kw}
    if proposals:
        kw.update(num_proposal_iterations=2, num_proposal_samples_per_ray=PROPOSAL_SAMPLES)
    else:
        kw.update(num_proposal_iterations=0)
    return small_config(num_nerf_samples_per_ray=1, implementation=impl, disable_scene_contraction=kind == "box", proposal_initial_sampler=sampler,
                        predict_normals=False, background_color=background, **kw)


def state(c, wide=False, proposals=False, background="last_sample"):
    """-> (cfg, sd: what the model loads, params: what the oracle reads, ocfg, rays) of a case; built once and shared."""
    from helpers import oracle_config, oracle_params_from_tcnn, synthetic_tcnn_checkpoint
    from signerf_amd import scene

    impl, levels, scale, kind, sampler = c
    key = ("state", c, wide, proposals, background)
    if key not in _CASES:
        cfg = config(impl, kind, sampler, wide, proposals, background)
        gain = {"head_gain": WIDE_HEAD_GAIN} if wide else {}
        if impl == "tcnn":
            assert scale == 1.0
            sd = no.keep_levels_tcnn(synthetic_tcnn_checkpoint(cfg, seed=0, **gain), levels, cfg)
            params = oracle_params_from_tcnn(sd, cfg)
        else:
            sd = no.keep_levels_torch(scene.synthetic_state_dict(cfg, seed=0, **gain), levels, cfg.log2_hashmap_size)
            if scale != 1.0:
                sd = dict(sd)
                sd[f"{no.P}.encoder.hash_table"] = sd[f"{no.P}.encoder.hash_table"] * scale
            params = sd
        if ("rays", kind) not in no._REFS:
            no._REFS["rays", kind] = no.sample_set(kind)
        _CASES[key] = (cfg, sd, params, oracle_config(cfg), no._REFS["rays", kind])
    return _CASES[key]


def reference(c, wide=False, background="last_sample"):
    """One case behind the uniform sampler: the fp32 oracle's render of the bundle (ref32) and the fp64 restatement at the oracle's own q,
    selector and bins (ref64) -> dict(ref32, ref64 {output: [N,C]}, oracle: its debug tensors, tau [N] fp64); computed once per case."""
    key = ("reference", c, wide, background)
    if key not in _CASES:
        _, _, params, ocfg, rays = state(c, wide, False, background)
        with torch.no_grad():
            out = onf.get_outputs(params, ocfg, rays["o"], rays["d"], rays["near"], rays["far"], return_debug=True)
        dbg = out["_debug"]
        bg = None if background == "last_sample" else {"white": WHITE}[background]
        r64 = sample(params, ocfg, dbg["q"][:, 0], dbg["selector"][:, 0], dbg["euclid_bins"], rays["d"], background=bg)
        _CASES[key] = {"ref32": {k: out[k] for k in OUTPUTS}, "ref64": {k: r64[k] for k in OUTPUTS}, "full64": r64, "oracle": dbg, "tau": r64["tau"][:, 0]}
    return _CASES[key]


def at_q(c, q, d, wide=False):
    """Behind the proposal sampler the kernel's own q is the only q there is: the colour of the sample at q [N,3] fp32 and direction d in fp64
    and in fp32 (the oracle at that q) -> (c64, c32) [N,3].  The selector does not enter the colour; a masked sample carries q = 0."""
    _, _, params, ocfg, _ = state(c, wide, True)
    c64 = colour(params, ocfg, d, density_h(params, ocfg, q), torch.float64)
    c32 = colour(params, ocfg, d, density_h(params, ocfg, q, torch.float32), torch.float32)
    return c64, c32


def all_cases():
    return no.all_cases()


case_id = no.case_id
