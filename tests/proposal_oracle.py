"""The proposal kernel (csrc/sn_proposal.h sn_proposal_kernel) per SAMPLE: the whole chain of a ray -- density of proposal net k
at the level's samples, alpha and transmittance, the level's median depth, the padded pdf and its inverse at the u grid, the spacing map back
to euclidean bins, the next level's positions -- restated for R rays in a given dtype.  fp64 is the reference the gate measures against; fp32
is oracle.nerfacto.get_outputs' own arithmetic (compared with it bit for bit on the CPU) and sets e_ref32.

The chain starts at GIVEN fp32 level-0 positions q0 (the oracle's, or the kernel's own position map at the oracle's level-0 bins) and at the
oracle's fp32 initial spacing and euclidean bins: level 0's cells and in-voxel offsets are decided from that fp32 q0, as tests/render_oracle.py
and tests/normals_oracle.py do; everything behind them -- blend, MLP, exponentials, cumsums, pdf, spacing maps, the later levels' positions and
cells -- runs in the dtype.  (oracle.nerfacto.get_outputs on .double() inputs is NOT a reference: its level-0 positions move across voxel
faces and its helpers mix dtypes.)

What a production launch lets a test read are the final euclidean bins (ops.render_with_final_bins), prop_depth_k and, for the default
variant, prop_q_k.  The final bins are a CONTINUOUS function of every proposal weight -- the inverse cdf is piecewise linear and the padding
keeps every pdf value positive, so a searchsorted tie moves no bin -- hence no sample is excluded and a max-norm gate applies.  The medians
are not continuous (a cumsum that passes 0.5 within rounding picks another bin): near_tie() marks those rays from the reference alone.

Single terms can be MUTATED (Mutant): tests/test_proposal_oracle_host.py feeds the mutants to the gate to show that it can fail."""
import dataclasses

import torch

import hashgrid_oracle as ho
import normals_oracle as no
import render_oracle as ro
import sampler_oracle as so
from helpers import onf
from oracle import tcnn_layout as tl

N_RAYS, FRAME = no.N_RAYS, no.FRAME
GATE_FACTOR = no.GATE_FACTOR       # the widest factor in use; an output starts at hashgrid_oracle.gate's 2 (DESIGN.md K2 holds the table)
DENSITY = 0.08                     # DENSE: every ray's cumulative weight crosses 0.5 at both levels
ONE = {"proposals": (16,), "main": 32}
TWO = {"proposals": (16, 8), "main": 16}
DENSE = {**TWO, "average_init_density": DENSITY}
SETTINGS = {"ONE": ONE, "TWO": TWO, "DENSE": DENSE}
ALL_DENSE_TCNN = [{"hidden_dim": 16, "log2_hashmap_size": 19, "num_levels": 5, "max_res": 64, "use_linear": False}] * 2   # 5 + 5 dense levels
TIE_FACTOR = 8                     # margin_k = TIE_FACTOR x max |cumsum32_k - cumsum64_k|


def PP(net):
    return f"proposal_networks.{net}.mlp_base"


@dataclasses.dataclass
class Mutant:
    """One wrong term of the chain, in proposal net `net` (None of them: the restatement itself)."""
    net: int = 0
    level: int = -1                       # the hash level the next four act on
    feature_factor: float = 1.0           # that level's blended features times this
    drop_cross_term: bool = False         # that level blended as A + ox B + oy C per z slice (render_oracle.coefficient_blend(cross=False))
    swap_corners: bool = False            # corners 1 <-> 3 exchanged at that level
    feat_scale: float = 1.0               # the power-of-two feature scale left off that level (its features / this)
    density_factor: float = 1.0           # sigma times this
    drop_abs_half: bool = False           # w relu(x) = (w x + w |x|) / 2 without its |x| half: relu(x) -> x / 2
    drop_hidden_bias: int = -1            # this hidden unit's bias taken as 0
    no_histogram_padding: bool = False    # histogram_padding not added to the weights
    drop_padding_term: bool = False       # the "+ padding / N" of the weights dropped (padding = relu(eps - sum) stays in the sum)
    inclusive_transmittance: bool = False  # the transmittance in front of a sample includes the sample's own tau
    u_without_offset: bool = False        # u = j / (M + 1) without its + 1 / (2 (M + 1))

    @property
    def touches_grid(self):
        return self.level >= 0 and (self.feature_factor != 1.0 or self.drop_cross_term or self.swap_corners or self.feat_scale != 1.0)


# ---- one proposal net at q ---------------------------------------------------------------------------------------------------------------------
def grid_of(params, ocfg, net):
    """normals_oracle.grid_of for proposal net `net`."""
    h = ocfg.proposals[net]
    if h.grid == "tcnn":
        meta = tl.grid_meta(h.num_levels, h.base_res, h.max_res, h.log2_hashmap_size, h.features_per_level)
        return {"kind": "tcnn", "table": params[f"{PP(net)}.encoder.tcnn_grid"], "meta": meta, "scales": torch.tensor(meta.scales, dtype=torch.float32),
                "level_rows": [(meta.offsets[k], meta.offsets[k + 1]) for k in range(h.num_levels)]}
    T = 1 << h.log2_hashmap_size
    return {"kind": "torch", "table": params[f"{PP(net)}.encoder.hash_table"], "log2_T": h.log2_hashmap_size,
            "scales": onf.hash_scalings(h.num_levels, h.base_res, h.max_res), "level_rows": [(k * T, (k + 1) * T) for k in range(h.num_levels)]}


_TCNN_ORDER = [ho.CORNERS.index("".join("c" if corner & (1 << a) else "f" for a in range(3))) for corner in range(8)]


def blend(kind, f, o):
    """The trilinear blend of the 8 corner rows f (hashgrid_oracle.CORNERS order) in their dtype, in the nesting of the grid's own oracle:
    oracle.nerfacto.hash_encode's (hashgrid_oracle.blend), or oracle/tcnn_layout.grid_encode's -- corners in bit order x y z, the weight a
    product started at 1, the sum started at 0 -- so that fp32 is that oracle's bits."""
    if kind == "torch":
        return ho.blend(f, o)
    acc = torch.zeros_like(f[0])
    for corner in range(8):
        weight = torch.ones_like(o[..., 0])
        for a in range(3):
            weight = weight * (o[..., a] if corner & (1 << a) else 1 - o[..., a])
        acc = acc + weight[..., None] * f[_TCNN_ORDER[corner]]
    return acc


def density(params, ocfg, net, q, q_cells, dtype, mutant=None):
    """-> (sigma [P] without the selector, h0 [P]) of proposal net `net`: cells and offsets from q_cells (fp32 at level 0, the dtype's q
    behind it), blend, the two mlp.layers and average_init_density exp(h0) in dtype."""
    m = mutant if (mutant is not None and mutant.net == net) else None
    grid = grid_of(params, ocfg, net)
    idx, off = no.cells(q_cells, grid)
    f, o = ho.gather(grid["table"].to(dtype), idx), off.to(dtype)
    if m is not None and m.touches_grid:
        k = m.level
        if m.swap_corners:
            f = [v.clone() for v in f]
            f[1][:, k], f[3][:, k] = f[3][:, k].clone(), f[1][:, k].clone()
        enc = blend(grid["kind"], f, o).clone()
        if m.drop_cross_term:
            enc[:, k] = ro.coefficient_blend([v[:, k] for v in f], o[:, k], cross=False)
        enc[:, k] *= m.feature_factor / m.feat_scale
    else:
        enc = blend(grid["kind"], f, o)
    W0, b0, W1, b1 = (params[f"{PP(net)}.mlp.layers.{i}.{w}"].to(dtype) for i in (0, 1) for w in ("weight", "bias"))
    if m is not None and m.drop_hidden_bias >= 0:
        b0 = b0.clone()
        b0[m.drop_hidden_bias] = 0
    z = torch.nn.functional.linear(enc.flatten(-2, -1), W0, b0)
    z = z / 2 if (m is not None and m.drop_abs_half) else torch.relu(z)
    h0 = torch.nn.functional.linear(z, W1, b1)[:, 0]
    sigma = ocfg.average_init_density * torch.exp(h0)
    if m is not None:
        sigma = sigma * m.density_factor
    return sigma, h0


# ---- weights, median, resampling -----------------------------------------------------------------------------------------------------------------
def weights_of(deltas, sigma, inclusive=False):
    """RaySamples.get_weights on [R,N] in the inputs' dtype (oracle.nerfacto.get_weights' operations in its order)."""
    tau = deltas * sigma
    alphas = 1 - onf._exp(-tau)
    if inclusive:
        trans = torch.cumsum(tau, dim=-1)
    else:
        trans = torch.cat([torch.zeros_like(tau[:, :1]), torch.cumsum(tau[:, :-1], dim=-1)], dim=-1)
    return torch.nan_to_num(alphas * onf._exp(-trans))


def median(weights, ebins):
    """DepthRenderer("median") -> (depth [R,1], cumsum [R,N])."""
    steps = (ebins[:, :-1] + ebins[:, 1:]) / 2
    cumulative = torch.cumsum(weights, dim=-1)
    idx = torch.searchsorted(cumulative, torch.full((weights.shape[0], 1), 0.5, dtype=weights.dtype), side="left")
    return torch.gather(steps, -1, torch.clamp(idx, 0, steps.shape[-1] - 1)), cumulative


def resample(sbins, weights, M, histogram_padding, dtype, mutant=None):
    """PDFSampler, eval mode: sampler_oracle.pdf_bins at oracle.nerfacto.pdf_u; with a mutant its restatement with that term wrong."""
    u = onf.pdf_u(M)
    if mutant is None or not (mutant.no_histogram_padding or mutant.drop_padding_term or mutant.u_without_offset):
        return so.pdf_bins(sbins, weights, u, histogram_padding=histogram_padding, dtype=dtype)[0]
    if mutant.u_without_offset:
        u = torch.linspace(0.0, 1.0 - (1.0 / (M + 1)), steps=M + 1)
    b, w = sbins.to(dtype), weights.to(dtype)
    if not mutant.no_histogram_padding:
        w = w + so._f32(histogram_padding)
    s = torch.sum(w, dim=-1, keepdim=True)
    padding = torch.relu(so._f32(1e-5) - s)
    if not mutant.drop_padding_term:
        w = w + padding / w.shape[-1]
    pdf = w / (s + padding)
    cdf = torch.min(torch.ones_like(pdf), torch.cumsum(pdf, dim=-1))
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], dim=-1)
    u = u.to(dtype).expand(cdf.shape[0], u.shape[-1]).contiguous()
    inds = torch.searchsorted(cdf, u, side="right")
    below, above = torch.clamp(inds - 1, 0, b.shape[-1] - 1), torch.clamp(inds, 0, b.shape[-1] - 1)
    c0, b0, c1, b1 = torch.gather(cdf, -1, below), torch.gather(b, -1, below), torch.gather(cdf, -1, above), torch.gather(b, -1, above)
    t = torch.clip(torch.nan_to_num((u - c0) / (c1 - c0), 0), 0, 1)
    return b0 + t * (b1 - b0)


def padding_case(R=130, N=16, seed=5):
    """Where the "+ padding / N" term lives: histogram_padding = 0 and rays without any weight (padding = relu(1e-5 - 0) = 1e-5, the pdf is
    uniform).  No render reaches it (a handle's histogram_padding is nerfacto's 0.01); ops.pdf_sample, which shares SnPdfNorm with the
    proposal kernel, does.  -> (spacing bins [R,N+1], weights [R,N]: a fifth of the rays all-zero, the others in [0.1, 1])."""
    g = torch.Generator().manual_seed(seed)
    sbins = so.initial_bins(torch.linspace(0.0, 1.0, N + 1), torch.rand(R, N + 1, generator=g))
    w = 0.1 + 0.9 * torch.rand(R, N, generator=g)
    w[::5] = 0.0
    return sbins, w


def selector_of(q):
    """The selector of selector-multiplied positions: a masked sample carries q = 0 (a NaN one is masked as well)."""
    return ((q > 0.0) & (q < 1.0)).all(dim=-1)


def chain(params, ocfg, rays, q0, dtype, mutant=None, dead=None):
    """K2 for R rays -> dict(levels: [dict(q, selector, density, weights, cumsum, median, sbins, ebins)], sbins, ebins: the final bins).
    q0 [R, N0, 3] fp32: the level-0 positions (selector-multiplied).  dead [R] bool: rays whose weights are 0 at every level, as the oracle
    gives for a ray with a NaN origin (nan_to_num); their q0 is not read."""
    assert q0.dtype == torch.float32 and q0.shape == (rays["o"].shape[0], ocfg.num_proposal_samples_per_ray[0], 3)
    n_prop = ocfg.num_proposal_iterations
    counts = list(ocfg.num_proposal_samples_per_ray[:n_prop]) + [ocfg.num_nerf_samples_per_ray]
    sampler, aabb = ocfg.proposal_initial_sampler, onf.scene_aabb(ocfg)
    o, d, near, far = (rays[k].to(dtype) for k in ("o", "d", "near", "far"))
    sb32, eb32 = onf.initial_sampler(rays["near"], rays["far"], counts[0], sampler)
    sbins, ebins = sb32.expand(o.shape[0], -1).to(dtype), eb32.to(dtype)
    if dead is not None:
        q0 = torch.where(dead[:, None, None], torch.zeros(()), q0)
    levels = []
    for k in range(n_prop):
        m = mutant if (mutant is not None and mutant.net == k) else None
        if k == 0:
            q_cells, q = q0, q0.to(dtype)
            sel = selector_of(q0)
        else:
            pos = onf.sample_positions(o, d, ebins[:, :-1, None], ebins[:, 1:, None])
            if dead is not None:
                pos = torch.where(dead[:, None, None], torch.zeros((), dtype=dtype), pos)
            q, sel = onf.normalized_positions(pos, aabb)
            q_cells = q
        sigma, _ = density(params, ocfg, k, q.reshape(-1, 3), q_cells.reshape(-1, 3), dtype, mutant)
        sigma = sigma.view(sel.shape) * sel
        w = weights_of(ebins[:, 1:] - ebins[:, :-1], sigma, inclusive=bool(m and m.inclusive_transmittance))
        if dead is not None:
            w = torch.where(dead[:, None], torch.zeros((), dtype=dtype), w)
        med, cum = median(w, ebins)
        levels.append({"q": q, "selector": sel, "density": sigma, "weights": w, "cumsum": cum, "median": med, "sbins": sbins, "ebins": ebins})
        sbins = resample(sbins, w, counts[k + 1], ocfg.histogram_padding, dtype, m)
        ebins = onf.spacing_to_euclidean(sbins, near, far, sampler)
    return {"levels": levels, "sbins": sbins, "ebins": ebins}


def gate(got, ref64, ref32, factor=GATE_FACTOR):
    """render_oracle.gate: max |got - ref64| <= factor x max |ref32 - ref64| + 1 ulp of the largest output, over everything."""
    return ro.gate(got.reshape(-1, 1), ref64.reshape(-1, 1), ref32.reshape(-1, 1), factor)


def near_tie(cum32, cum64):
    """-> (rays [R] bool whose fp64 cumsum passes within margin of 0.5 at some sample, margin = TIE_FACTOR x max |cumsum32 - cumsum64|):
    there another arithmetic may pick another median bin.  From the two restatements alone."""
    margin = TIE_FACTOR * float((cum32.double() - cum64).abs().max())
    return ((cum64 - 0.5).abs() <= margin).any(-1), margin


# ---- the state dicts of the cases ---------------------------------------------------------------------------------------------------------------
def keep_prop_levels_torch(sd, net, levels, cfg):
    """The state dict with every level of proposal net `net`'s hash table zeroed except `levels` (None: all of them stay)."""
    if levels is None:
        return sd
    sd, key, log2_T = dict(sd), f"{PP(net)}.encoder.hash_table", cfg.proposal_net_args_list[net]["log2_hashmap_size"]
    t = torch.zeros_like(sd[key])
    for k in levels:
        t[k << log2_T:(k + 1) << log2_T] = sd[key][k << log2_T:(k + 1) << log2_T]
    sd[key] = t
    return sd


def keep_prop_levels_tcnn(sd, net, levels, cfg):
    """The same for a tiny-cuda-nn checkpoint: the grid rows follow the network matrices in the module's flat vector."""
    if levels is None:
        return sd
    sd, key, a = dict(sd), f"{PP(net)}.tcnn_encoding.params", cfg.proposal_net_args_list[net]
    meta = tl.grid_meta(a["num_levels"], a.get("base_res", 16), a["max_res"], a["log2_hashmap_size"])
    flat = sd[key].clone()
    rows = flat[tl.mlp_n_params(2 * a["num_levels"], a["hidden_dim"], 2, 1):].view(meta.n_rows, 2)
    live = torch.zeros(meta.n_rows, dtype=torch.bool)
    for k in levels:
        live[meta.offsets[k]:meta.offsets[k + 1]] = True
    rows[~live] = 0
    sd[key] = flat
    return sd


def keep_prop_levels(sd, net, levels, cfg):
    return (keep_prop_levels_torch if cfg.implementation == "torch" else keep_prop_levels_tcnn)(sd, net, levels, cfg)


# ---- the cases (shared by the host tests and tests/test_gpu_proposal_samples.py) -----------------------------------------------------------------
# A case: (impl, kind, sampler, setting name, keep: None or (net, levels), scale, nets: None or a proposal_net_args_list)
_CASES = {}


def case(impl="torch", kind="contract", sampler="piecewise", setting="TWO", keep=None, scale=1.0, nets=None):
    return (impl, kind, sampler, setting, keep, scale, nets)


def case_id(c):
    impl, kind, sampler, setting, keep, scale, nets = c
    parts = [impl, setting] + ([kind] if kind != "contract" else []) + ([sampler] if sampler != "piecewise" else [])
    if keep is not None:
        parts.append(f"net{keep[0]}-L" + "+".join(str(k) for k in keep[1]))
    return "-".join(parts + ([f"x{scale:g}"] if scale != 1.0 else []) + ([nets] if nets else []))


def config(impl="torch", kind="contract", sampler="piecewise", setting="TWO", nets=None, **kw):
    """The model config of a case: per-ray nears / fars come with the rays; no normals; small_config's tables (or `nets`)."""
    from helpers import small_config

    s = SETTINGS[setting]
    if "average_init_density" in s:
        kw.setdefault("average_init_density", s["average_init_density"])
    if nets == "all-dense":
        kw["proposal_net_args_list"] = [dict(a) for a in ALL_DENSE_TCNN]
    return small_config(num_proposal_iterations=len(s["proposals"]), num_proposal_samples_per_ray=s["proposals"], num_nerf_samples_per_ray=s["main"],
                        implementation=impl, disable_scene_contraction=kind == "box", proposal_initial_sampler=sampler, predict_normals=False, **kw)


def state(c):
    """-> (cfg, sd: what the model loads, params: what the oracle reads, ocfg, rays) of a case; built once and shared."""
    from helpers import oracle_config, oracle_params_from_tcnn, synthetic_tcnn_checkpoint
    from signerf_amd import scene

    impl, kind, sampler, setting, keep, scale, nets = c
    key = ("state", c)
    if key not in _CASES:
        cfg = config(impl, kind, sampler, setting, nets)
        sd = synthetic_tcnn_checkpoint(cfg, seed=0) if impl == "tcnn" else scene.synthetic_state_dict(cfg, seed=0)
        if keep is not None:
            sd = keep_prop_levels(sd, keep[0], keep[1], cfg)
        if scale != 1.0:
            assert impl == "torch"
            sd = dict(sd)
            for net in range(cfg.num_proposal_iterations):
                sd[f"{PP(net)}.encoder.hash_table"] = sd[f"{PP(net)}.encoder.hash_table"] * scale
        params = oracle_params_from_tcnn(sd, cfg) if impl == "tcnn" else sd
        if ("rays", kind) not in no._REFS:
            no._REFS["rays", kind] = no.sample_set(kind)
        _CASES[key] = (cfg, sd, params, oracle_config(cfg), no._REFS["rays", kind])
    return _CASES[key]


def oracle_outputs(c):
    """oracle.nerfacto.get_outputs of the case's bundle with its debug tensors; computed once per case."""
    key = ("oracle", c)
    if key not in _CASES:
        _, _, params, ocfg, rays = state(c)
        with torch.no_grad():
            _CASES[key] = onf.get_outputs(params, ocfg, rays["o"], rays["d"], rays["near"], rays["far"], return_debug=True)
    return _CASES[key]


def level0_bins(c):
    """The oracle's fp32 euclidean bins of level 0 [R, N0 + 1]."""
    _, _, _, ocfg, rays = state(c)
    return onf.initial_sampler(rays["near"], rays["far"], ocfg.num_proposal_samples_per_ray[0], ocfg.proposal_initial_sampler)[1]


def references(c, q0=None, dead=None):
    """-> (chain in fp64, chain in fp32) at q0 (None: the oracle's own prop_q_0, cached)."""
    _, _, params, ocfg, rays = state(c)
    if q0 is None:
        key = ("references", c)
        if key not in _CASES:
            q = oracle_outputs(c)["_debug"]["prop_q_0"]
            _CASES[key] = (chain(params, ocfg, rays, q, torch.float64), chain(params, ocfg, rays, q, torch.float32))
        return _CASES[key]
    return chain(params, ocfg, rays, q0, torch.float64, dead=dead), chain(params, ocfg, rays, q0, torch.float32, dead=dead)
