"""The normals kernel (csrc/sn_normals.h) per SAMPLE: with one sample per ray ("num_nerf_samples_per_ray=1", no proposal
nets, per-ray nears / fars) the rendered "normals" of a ray ARE its sample's (-g / |g| + 1) / 2 -- the weight cancels in the
renormalisation -- and a hash table with all but one or two levels zeroed makes the direction come from those levels' slope code alone.

This module restates the two outputs in a given dtype (fp64: the reference the gate measures against; fp32: what is compared with the
oracle's autograd on the CPU).  The normalised positions q are the fp32 oracle's, never recomputed (that would move samples across voxel
faces): indices and in-voxel offsets come from fp32 q (tests/hashgrid_oracle.cells, oracle/tcnn_layout's arithmetic), everything behind
them runs in the dtype.  The slopes of the blend are written out by hand (the formulas the kernel implements), so that single terms can be
MUTATED: the host tests feed the mutants to the gate to show that it can fail.  `ambiguous` marks, from the reference alone, the samples
whose normal is decided by a tie (a layer-1 pre-activation at 0, a position within 2 ulp of a voxel face)."""
import dataclasses
import math

import torch

import hashgrid_oracle as ho
from helpers import onf
from oracle import tcnn_layout as tl

N_RAYS = 4165           # 65 waves and 5 lanes (flat bundle); 49 x 85 as a frame: 8x8 tiles with ragged edges on both axes
FRAME = (49, 85)
N_CONTRACTED, N_FAR, N_LATTICE = 200, 30, 63
TIE_REL = 1e-5          # ReLU tie: |z1_j| below this share of sum_k |W0_jk enc_k| + |b0_j|
FACE_ULPS = 2           # near a face: fl32(q s) within this many of its own ulps of an integer, without being one
MAX_EXCLUDED = 0.02
MIN_WEIGHT = 1e-3
P = "field.mlp_base"


@dataclasses.dataclass
class Mutant:
    """One wrong term of the analytic normal (None of them: the restatement itself)."""
    slope_level: int = -1        # this level's slopes times slope_factor
    slope_factor: float = 1.0
    negate_dz: tuple = ()        # (level, feature): d / d oz of that feature negated
    keep_zero_offset: bool = False   # torch grid: the ceil corner taken as floor + 1, so an offset of exactly 0 keeps its slope
    swap_corners_level: int = -1     # corners 1 <-> 3 exchanged at this level
    ignore_relu_unit: int = -1       # this layer-1 unit's ReLU mask taken as 1


# ---- the sample set ------------------------------------------------------------------------------------------------------------------------
def sample_set(kind="contract", seed=3):
    """-> dict(o, d [N,3], near, far [N,1], far_rows, lattice [N] bool).  kind "contract": positions U(-1.5, 1.5)^3, 200 rows times 4 (the
    contraction branch), 30 rows with coordinates of order 1e2 / 1e4 / 1e6 (q within 1e-6 of 0 or 1: the last cell of the de-hashed copies)
    and a block of lattice points hit exactly, with in-voxel offsets of exactly 0 on 1, 2 and 3 axes of level 0.  kind "box": positions
    inside the scene box [-1, 1]^3 for disable_scene_contraction (no far rows), the same lattice block.  Rays: t in [1, 2),
    near = 0.75 t, far = 1.25 t, o = p - d t; lattice rows: d along an axis, o = p - d, near 0.75, far 1.25 (every step exact)."""
    g = torch.Generator().manual_seed(seed)
    N = N_RAYS
    box = kind == "box"
    p = (torch.rand(N, 3, generator=g) * 2 - 1) * (0.999 if box else 1.5)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    t = 1 + torch.rand(N, 1, generator=g)
    far_rows = torch.zeros(N, dtype=torch.bool)
    if not box:
        p[:N_CONTRACTED] *= 4
        mag = torch.tensor([1e2, 1e4, 1e6]).repeat_interleave(N_FAR // 3)
        sign = torch.where(torch.rand(N_FAR, 3, generator=g) < 0.5, -1.0, 1.0)
        p[N_CONTRACTED:N_CONTRACTED + N_FAR] = sign * mag[:, None] * (0.5 + torch.rand(N_FAR, 3, generator=g))
        far_rows[N_CONTRACTED:N_CONTRACTED + N_FAR] = True
    lo = N_CONTRACTED + N_FAR
    lattice = torch.zeros(N, dtype=torch.bool)
    lattice[lo:lo + N_LATTICE] = True
    # q = j / 16 on the zero-offset axes, j / 16 + a multiple of 2^-12 on the others: |p| < 1 (no contraction), every operation exact
    j = torch.randint(5, 12, (N_LATTICE, 3), generator=g).float()
    frac = torch.randint(1, 255, (N_LATTICE, 3), generator=g).float() / 4096
    n_zero = 1 + torch.arange(N_LATTICE) % 3                                   # 1, 2, 3 axes with offset 0 ...
    first = (torch.arange(N_LATTICE) // 3) % 3                                 # ... starting at this axis
    axes = (torch.arange(3)[None, :] - first[:, None]) % 3                     # axis a is the ((a - first) % 3)-th
    qv = j / 16 + torch.where(axes < n_zero[:, None], torch.zeros(()), frac)
    pl = (qv * 2 - 1) if box else (qv * 4 - 2)
    dl = torch.zeros(N_LATTICE, 3)
    dl[torch.arange(N_LATTICE), (torch.arange(N_LATTICE) // 9) % 3] = torch.where(torch.arange(N_LATTICE) % 2 == 0, 1.0, -1.0)
    p[lattice], d[lattice], t[lattice] = pl, dl, 1.0
    o = p - d * t
    return {"o": o, "d": d, "near": 0.75 * t, "far": 1.25 * t, "far_rows": far_rows, "lattice": lattice, "kind": kind}


# ---- cells: table rows and in-voxel offsets of the 8 corners, in q's dtype (fp32: the oracles' own arithmetic) ---------------------------------
def grid_of(params, ocfg):
    """-> dict(kind, table [rows, 2], scales [L] fp32, log2_T / meta)."""
    h = ocfg.main
    if h.grid == "tcnn":
        meta = tl.grid_meta(h.num_levels, h.base_res, h.max_res, h.log2_hashmap_size, h.features_per_level)
        return {"kind": "tcnn", "table": params[f"{P}.encoder.tcnn_grid"], "meta": meta, "scales": torch.tensor(meta.scales, dtype=torch.float32),
                "level_rows": [(meta.offsets[k], meta.offsets[k + 1]) for k in range(h.num_levels)]}
    T = 1 << h.log2_hashmap_size
    return {"kind": "torch", "table": params[f"{P}.encoder.hash_table"], "log2_T": h.log2_hashmap_size,
            "scales": onf.hash_scalings(h.num_levels, h.base_res, h.max_res), "level_rows": [(k * T, (k + 1) * T) for k in range(h.num_levels)]}


def scaled_positions(q, grid):
    """x [N,L,3] in q's dtype: q s (torch grid), fmaf(s, q, 0.5) (tiny-cuda-nn grid) -- in fp32 exactly what the oracles compute."""
    s = grid["scales"]
    if grid["kind"] == "torch":
        return q[..., None, :] * s.to(q.dtype).view(-1, 1)
    return (q.double()[..., None, :] * s.double().view(-1, 1) + 0.5).to(q.dtype)


def cells(q, grid, keep_zero_offset=False):
    """-> (idx [N,L,8] int64 in the order of hashgrid_oracle.CORNERS, offset [N,L,3] in q's dtype)."""
    if grid["kind"] == "torch":
        sf, sc, idx, offset = onf.hash_corner_indices(q, grid["scales"].to(q.dtype), grid["log2_T"])
        if keep_zero_offset:    # the mutant: what a kernel that fetches floor + 1 computes without the 0 / 1 factor
            sc = sf + 1
            T = 1 << grid["log2_T"]
            lvl = torch.arange(grid["scales"].numel()) * T
            pick = lambda c: torch.stack([(sc if c[a] == "c" else sf)[..., a] for a in range(3)], -1)  # noqa: E731
            idx = torch.stack([onf.hash_fn(pick(c), T, lvl) for c in ho.CORNERS], -1)
        return idx, offset
    meta = grid["meta"]
    x = scaled_positions(q, grid)
    fl = torch.floor(x)
    base = fl.to(torch.int64)
    idx = torch.stack([torch.stack([tl.grid_rows(meta, k, base[:, k] + torch.tensor([int(c[a] == "c") for a in range(3)])) + meta.offsets[k]
                                    for k in range(meta.num_levels)], 1) for c in ho.CORNERS], -1)
    return idx, x - fl


def level_slopes(f, o, mutant=None):
    """The literal derivative of hashgrid_oracle.blend in the offsets: f the 8 corner rows [N,L,F], o [N,L,3] -> dx, dy, dz [N,L,F]."""
    if mutant is not None and mutant.swap_corners_level >= 0:
        f = [v.clone() for v in f]
        k = mutant.swap_corners_level
        f[1][:, k], f[3][:, k] = f[3][:, k].clone(), f[1][:, k].clone()
    ox, oy, oz = o[..., 0:1], o[..., 1:2], o[..., 2:3]
    f_03, f_12 = f[0] * ox + f[3] * (1 - ox), f[1] * ox + f[2] * (1 - ox)
    f_56, f_47 = f[5] * ox + f[6] * (1 - ox), f[4] * ox + f[7] * (1 - ox)
    dx = ((f[0] - f[3]) * oy + (f[1] - f[2]) * (1 - oy)) * oz + ((f[4] - f[7]) * oy + (f[5] - f[6]) * (1 - oy)) * (1 - oz)
    dy = (f_03 - f_12) * oz + (f_47 - f_56) * (1 - oz)
    dz = (f_03 * oy + f_12 * (1 - oy)) - (f_47 * oy + f_56 * (1 - oy))
    if mutant is not None and mutant.negate_dz:
        dz = dz.clone()
        dz[:, mutant.negate_dz[0], mutant.negate_dz[1]] *= -1
    return dx, dy, dz


def _mlp0(params, dtype):
    return [params[f"{P}.mlp.layers.{i}.{w}"].to(dtype) for i in (0, 1) for w in ("weight", "bias")]


def density_h(params, ocfg, q, dtype=torch.float64):
    """h [N,16] (pre-activation density, then the geometry features), z1 [N,64], enc [N,32]: the blend and the MLP in dtype at fp32-decided cells."""
    grid = grid_of(params, ocfg)
    idx, off = cells(q, grid)
    enc = ho.blend(ho.gather(grid["table"].to(dtype), idx), off.to(dtype)).flatten(-2, -1)
    W0, b0, W1, b1 = _mlp0(params, dtype)
    z1 = enc @ W0.T + b0
    return torch.relu(z1) @ W1.T + b1, z1, enc


def analytic(params, ocfg, q, dtype=torch.float64, mutant=None):
    """Field.get_normals by hand: g_feat = W0^T (W1[0, :] * [z1 > 0]), g_q = sum_l s_l g_feat . d blend / d offset, n = -g_q / max(|g_q|, 1e-12).
    -> dict(n [N,3], g_q, z1, enc, h) in dtype.  (q in fp64 as well: cells and all in fp64, for the finite-difference check alone.)"""
    assert q.dtype in (torch.float32, dtype)
    grid = grid_of(params, ocfg)
    h, z1, enc = density_h(params, ocfg, q, dtype)
    W0, _, W1, _ = _mlp0(params, dtype)
    mask = (z1 > 0).to(dtype)
    if mutant is not None and mutant.ignore_relu_unit >= 0:
        mask[:, mutant.ignore_relu_unit] = 1
    g_feat = (W1[0] * mask) @ W0
    idx, off = cells(q, grid, keep_zero_offset=bool(mutant and mutant.keep_zero_offset))
    dx, dy, dz = level_slopes(ho.gather(grid["table"].to(dtype), idx), off.to(dtype), mutant)
    g = g_feat.view(q.shape[0], -1, dx.shape[-1])
    d = torch.stack([(g * dx).sum(-1), (g * dy).sum(-1), (g * dz).sum(-1)], -1) * grid["scales"].to(dtype).view(1, -1, 1)       # [N,L,3]
    if mutant is not None and mutant.slope_level >= 0:
        d[:, mutant.slope_level] *= mutant.slope_factor
    g_q = d.sum(1)
    n = -g_q / g_q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return {"n": n, "g_q": g_q, "z1": z1, "enc": enc, "h": h}


def frequency_encoding(x, grid_kind):
    """The position encoding of the pred-normal MLP in x's dtype.  torch grid: nerfstudio's NeRFEncoding, sin(2 pi x 2^k) for (axis, k), then
    the same a quarter period on; tiny-cuda-nn: its Frequency encoding in oracle/tcnn_layout.frequency_encoding's order (which returns
    fp32: the host tests hold this function, rounded, against it bit for bit)."""
    if grid_kind == "torch":
        si = (2.0 * math.pi * x)[..., None] * torch.tensor([1.0, 2.0], dtype=x.dtype)
        si = si.reshape(*x.shape[:-1], -1)
        return torch.sin(torch.cat([si, si + math.pi / 2.0], dim=-1))
    outs = []
    for i in range(x.shape[-1]):
        for f in range(2):
            arg = x[:, i].double() * (2.0**f) * math.pi
            outs += [torch.sin(arg), torch.sin(arg + math.pi / 2.0)]
    return torch.stack(outs, dim=-1).to(x.dtype)


def predicted(params, ocfg, pos, h, dtype=torch.float64):
    """NerfactoField's pred-normal branch: [encoding of the fp32 WORLD position (12) | geometry features h[:, 1:16]] -> 27 -> 64 -> 64 -> 64
    -> Linear(64, 3), tanh, F.normalize.  -> [N,3] in dtype."""
    assert pos.dtype == torch.float32
    x = torch.cat([frequency_encoding(pos.to(dtype), ocfg.main.grid), h[:, 1:1 + ocfg.geo_feat_dim].to(dtype)], dim=-1)
    for i in range(3):
        x = x @ params[f"field.mlp_pred_normals.layers.{i}.weight"].to(dtype).T + params[f"field.mlp_pred_normals.layers.{i}.bias"].to(dtype)
        if i < 2:
            x = torch.relu(x)
    x = torch.tanh(x @ params["field.field_head_pred_normals.net.weight"].to(dtype).T + params["field.field_head_pred_normals.net.bias"].to(dtype))
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def rendered(n, w):
    """NormalsRenderer + NormalsShader for ONE sample of weight w [N,1]: m = w n, (m / (|m| + 1e-10) + 1) / 2."""
    m = w.to(n.dtype) * n
    return (m / (m.norm(dim=-1, keepdim=True) + 1e-10) + 1) / 2


# ---- which samples a tie decides -------------------------------------------------------------------------------------------------------------
def live_levels(grid):
    return [k for k, (a, b) in enumerate(grid["level_rows"]) if bool((grid["table"][a:b] != 0).any())]


def exact_face(q, grid):
    """[N] bool: an in-voxel offset of exactly 0 on some axis of some live level -- a designed case, NOT ambiguous (the torch grid drops
    that axis' slope; on the tiny-cuda-nn grid floor + 1 is a different row and nothing is special)."""
    x = scaled_positions(q, grid)[:, live_levels(grid)]
    return (x == torch.floor(x)).flatten(1).any(1)


def ambiguous(params, ocfg, q, ref=None):
    """-> (relu_tie [N] bool, near_face [N] bool), from the fp64 reference alone."""
    grid = grid_of(params, ocfg)
    ref = ref or analytic(params, ocfg, q)
    W0, b0, _, _ = _mlp0(params, torch.float64)
    scale = ref["enc"].abs() @ W0.abs().T + b0.abs()
    relu_tie = ((ref["z1"].abs() / scale.clamp_min(1e-300)) < TIE_REL).any(1)
    x = scaled_positions(q, grid)[:, live_levels(grid)]                        # fp32
    ulp = torch.ldexp(torch.ones(()), torch.frexp(x.abs().clamp_min(2.0**-126))[1] - 24)
    dist = (x - torch.round(x)).abs()
    near_face = ((dist > 0) & (dist <= FACE_ULPS * ulp)).flatten(1).any(1)
    return relu_tie, near_face


# ---- one case: the fp32 oracle's render of the bundle and the fp64 reference of both outputs ----------------------------------------------------
def reference(params, ocfg, rays):
    """-> dict: ref32 / ref64 {"normals", "pred_normals"} [N,3] in the rendered [0, 1] form, keep [N] bool (what the gate compares),
    relu_tie, near_face, exact_face [N] bool, q, pos, weights."""
    ocfg = dataclasses.replace(ocfg, predict_normals=True)
    assert ocfg.num_nerf_samples_per_ray == 1 and ocfg.num_proposal_iterations == 0
    with torch.no_grad():
        out = onf.get_outputs(params, ocfg, rays["o"], rays["d"], rays["near"], rays["far"], return_debug=True)
    dbg = out["_debug"]
    q, w = dbg["q"][:, 0], dbg["weights"][:, 0].double()
    eb = dbg["euclid_bins"]    # (the sampler's own round trip through the spacing function: not nears / fars bit for bit)
    pos = onf.sample_positions(rays["o"], rays["d"], eb[:, :-1, None], eb[:, 1:, None])[:, 0]
    ref = analytic(params, ocfg, q)
    relu_tie, near_face = ambiguous(params, ocfg, q, ref)
    ref64 = {"normals": rendered(ref["n"], w), "pred_normals": rendered(predicted(params, ocfg, pos, ref["h"]), w)}
    return {"ref32": {k: out[k] for k in ref64}, "ref64": ref64, "keep": ~(relu_tie | near_face), "relu_tie": relu_tie, "near_face": near_face,
            "exact_face": exact_face(q, grid_of(params, ocfg)), "q": q, "pos": pos, "weights": w, "selector": dbg["selector"][:, 0],
            "starts": eb[:, 0], "ends": eb[:, 1]}


# The project's gate has factor 2.  This kernel's lerps are fmaf chains on differences, its reciprocals have 1 ulp and its split-precision
# products two terms, and both errors are maxima over 4165 samples that the few ill-conditioned ones (a gradient that nearly cancels)
# decide: measured e_hip / e_ref32 over every case of tests/test_gpu_normals_samples.py is at most 7.1 (DESIGN.md K3 holds the table), so
# the factor is the next power of two, 8; a ratio beyond 8 is a finding to explain from the code, not a tolerance to widen.
GATE_FACTOR = 8


def gate(got, ref64, ref32, rows, factor=GATE_FACTOR):
    """hashgrid_oracle.gate with GATE_FACTOR in place of its 2 (e_hip <= factor x e_ref32 + 1 ulp of the largest output) on the samples `rows` -> (ok, e_hip, e_ref32, the limit).
    e_ref32 is the fp32 oracle's own error against the fp64 reference, never the kernel's."""
    _, e_hip, e_ref, limit = ho.gate(got[rows].double(), ref64[rows], ref32[rows])
    limit = factor * e_ref + (limit - 2 * e_ref)
    return e_hip <= limit, e_hip, e_ref, limit


def h0_at(params, ocfg, q):
    """The pre-activation density at q of ANY dtype, cells included (the finite-difference check moves q in fp64) -> (h0 [N], z1 > 0)."""
    grid = grid_of(params, ocfg)
    idx, off = cells(q, grid)
    enc = ho.blend(ho.gather(grid["table"].to(q.dtype), idx), off).flatten(-2, -1)
    W0, b0, W1, b1 = _mlp0(params, q.dtype)
    z1 = enc @ W0.T + b0
    return torch.relu(z1) @ W1[0] + b1[0], z1 > 0


# ---- the state dicts of the cases ---------------------------------------------------------------------------------------------------------------
def keep_levels_torch(sd, levels, log2_T):
    """The state dict with every level of the main hash table zeroed except `levels` (None: all of them stay)."""
    if levels is None:
        return sd
    sd = dict(sd)
    t = torch.zeros_like(sd[f"{P}.encoder.hash_table"])
    for k in levels:
        t[k << log2_T:(k + 1) << log2_T] = sd[f"{P}.encoder.hash_table"][k << log2_T:(k + 1) << log2_T]
    sd[f"{P}.encoder.hash_table"] = t
    return sd


def keep_levels_tcnn(sd, levels, cfg):
    """The same for a tiny-cuda-nn checkpoint: the grid rows follow the network matrices in the module's flat vector."""
    if levels is None:
        return sd
    sd = dict(sd)
    meta = tl.grid_meta(cfg.num_levels, cfg.base_res, cfg.max_res, cfg.log2_hashmap_size)
    flat = sd[f"{P}.tcnn_encoding.params"].clone()
    n_net = tl.mlp_n_params(2 * cfg.num_levels, cfg.hidden_dim, 2, 16)
    rows = flat[n_net:].view(meta.n_rows, 2)
    live = torch.zeros(meta.n_rows, dtype=torch.bool)
    for k in levels:
        live[meta.offsets[k]:meta.offsets[k + 1]] = True
    rows[~live] = 0
    sd[f"{P}.tcnn_encoding.params"] = flat
    return sd


# ---- the cases (shared by the host tests and tests/test_gpu_normals_samples.py) --------------------------------------------------------------
SINGLES = [(k,) for k in range(16)]
PAIRS = [(k, k + 1) for k in range(15)]            # 6|7 re-gathered / kept, 8|9 coefficient / plain copy, 10|11 copy / hashed
BOUNDARY = [(6, 7), (8, 9), (10, 11), (0,), (9,), (11,), (15,)]
TCNN_LEVELS = [(0,), (1,), (2,), (15,), (1, 2)]    # 0, 1: indexed densely at T = 2^14; 2, 15: hashed
_REFS = {}


def config(impl="torch", kind="contract", sampler="piecewise", **kw):
    from helpers import small_config

    if impl == "tcnn":
        kw.setdefault("average_init_density", 3.0)         # bias-free nets: the opacity comes from here (tests/test_gpu_tcnn.py)
    return small_config(num_proposal_iterations=0, num_nerf_samples_per_ray=1, implementation=impl, disable_scene_contraction=kind == "box",
                        proposal_initial_sampler=sampler, **kw)


def case(impl="torch", levels=None, scale=1.0, kind="contract", sampler="piecewise"):
    """-> (sd: what the model loads, params: what the oracle reads, ocfg, rays, ref: reference(...) -- computed once per case and shared)."""
    from helpers import oracle_config, oracle_params_from_tcnn, synthetic_tcnn_checkpoint
    from signerf_amd import scene

    cfg = config(impl, kind, sampler)
    if impl == "tcnn":
        assert scale == 1.0
        sd = keep_levels_tcnn(synthetic_tcnn_checkpoint(cfg, seed=0), levels, cfg)
        params = oracle_params_from_tcnn(sd, cfg)
    else:
        sd = keep_levels_torch(scene.synthetic_state_dict(cfg, seed=0), levels, cfg.log2_hashmap_size)
        if scale != 1.0:
            sd = dict(sd)
            sd[f"{P}.encoder.hash_table"] = sd[f"{P}.encoder.hash_table"] * scale
        params = sd
    ocfg = dataclasses.replace(oracle_config(cfg), predict_normals=True)
    key = (impl, levels, scale, kind, sampler)
    if ("rays", kind) not in _REFS:
        _REFS["rays", kind] = sample_set(kind)
    rays = _REFS["rays", kind]
    if key not in _REFS:
        _REFS[key] = reference(params, ocfg, rays)
    return sd, params, ocfg, rays, _REFS[key]


def all_cases():
    """Every (impl, levels, scale, kind, sampler) the GPU tests render (precision and the de-hashed copies do not enter the reference)."""
    out = [("torch", lv, 1.0, "contract", "piecewise") for lv in [None] + SINGLES + PAIRS]
    out += [("torch", None, 1e-3, "contract", "piecewise"), ("torch", None, 1.0, "box", "piecewise"), ("torch", None, 1.0, "contract", "uniform")]
    out += [("tcnn", lv, 1.0, "contract", "piecewise") for lv in [None] + TCNN_LEVELS]
    return out


def case_id(c):
    impl, lv, scale, kind, sampler = c
    name = "all" if lv is None else "L" + "+".join(str(k) for k in lv)
    return "-".join([impl, name] + ([f"x{scale:g}"] if scale != 1.0 else []) + ([kind] if kind != "contract" else []) + ([sampler] if sampler != "piecewise" else []))
