"""Training-mode proposal sampling restated as plain torch ops, generic in dtype: nerfstudio's ``SpacedSampler`` and ``PDFSampler`` in their
training branch (stratified jitter, ``include_original=False``) [NS-RECALL, nerfstudio 1.0.2 ``model_components/ray_samplers.py``], the
per-sample quantities of a ``RaySamples`` and the Philox4x32-10 generator csrc/sn_sampler.h draws from.  In fp32 this is what the
kernels are compared with bit for bit (everything but the cdf) and what sets the error scale of the cdf; in fp64 it is the reference.

The inputs are fp32 numbers whatever the dtype of the arithmetic: scalars (padding, anneal, eps) are rounded to fp32 first.
"""
import numpy as np
import torch

from helpers import onf

MODES = ("piecewise", "uniform")     # spacing_mode 0 / 1
M0, M1 = 0xD2511F53, 0xCD9E8D57      # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85      # key increments (golden ratio, sqrt(3) - 1)


def _f32(x: float) -> float:
    return float(np.float32(x))


# ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (broadcastable), key: 2 -> the 4 result words, uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(0xFFFFFFFF), p1 >> np.uint64(32), p1 & np.uint64(0xFFFFFFFF)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def word_to_float(x) -> np.ndarray:
    """(x >> 8) * 2^-24: 24 random bits, in [0, 1), exact in fp32."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0**-24)).astype(np.float32)


def philox_uniform(R: int, n_edges: int, seed: int, offset: int, single_jitter: bool) -> torch.Tensor:
    """The numbers a seeded launch uses: counter (ray, j, offset_lo, offset_hi), key (seed_lo, seed_hi), word 0.  [R] under single jitter
    (j = 0), else [R, n_edges]."""
    ray = np.arange(R, dtype=np.uint64)
    if single_jitter:
        ctr = (ray, np.zeros(R, np.uint64), offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF)
    else:
        ctr = (ray[:, None], np.arange(n_edges, dtype=np.uint64)[None, :], offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF)
    w0 = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[0]
    return torch.from_numpy(word_to_float(w0))


# ---- the samplers ----------------------------------------------------------------------------------------------------------------------------
def _jitter(rand: torch.Tensor, dtype) -> torch.Tensor:
    """[R] (single jitter) -> [R,1]; [R,J] stays."""
    rand = rand.to(dtype)
    return rand[:, None] if rand.ndim == 1 else rand


def euclid(bins, nears, fars, mode: str, dtype=torch.float32):
    """spacing_to_euclidean_fn: s^-1(bins s_far + (1 - bins) s_near); nears, fars [R]."""
    return onf.spacing_to_euclidean(bins.to(dtype), nears.to(dtype)[:, None], fars.to(dtype)[:, None], mode)


def initial_bins(base_bins, rand, dtype=torch.float32):
    """SpacedSampler, training branch: base_bins [N+1] (linspace(0, 1, N+1)), rand [R] or [R,N+1] -> spacing bins [R,N+1]."""
    bins = base_bins.to(dtype)[None, :]
    centers = (bins[..., 1:] + bins[..., :-1]) / 2.0
    upper = torch.cat([centers, bins[..., -1:]], -1)
    lower = torch.cat([bins[..., :1], centers], -1)
    return lower + (upper - lower) * _jitter(rand, dtype)


def u_grid(M: int) -> torch.Tensor:
    return torch.linspace(0.0, 1.0 - (1.0 / (M + 1)), steps=M + 1)


def train_u(grid, rand, dtype=torch.float32):
    """u = grid + rand / (M + 1): grid [M+1], rand [R] or [R,M+1] -> [R,M+1]."""
    nb = grid.shape[0]
    r = _jitter(rand, dtype) / nb
    return (grid.to(dtype)[None, :] + r).expand(r.shape[0], nb).contiguous()


def pdf_bins(existing_bins, weights, u, anneal: float = 1.0, histogram_padding: float = 0.01, eps: float = 1e-5, dtype=torch.float32):
    """PDFSampler: existing_bins [R,N+1], weights [R,N], u [R,M+1] (or [M+1]) -> (bins [R,M+1], inds, cdf)."""
    b, w = existing_bins.to(dtype), weights.to(dtype)
    if _f32(anneal) != 1.0:
        w = torch.pow(w, _f32(anneal))
    w = w + _f32(histogram_padding)
    s = torch.sum(w, dim=-1, keepdim=True)
    padding = torch.relu(_f32(eps) - s)
    w = w + padding / w.shape[-1]
    s = s + padding
    pdf = w / s
    cdf = torch.min(torch.ones_like(pdf), torch.cumsum(pdf, dim=-1))
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], dim=-1)
    u = u.to(dtype).expand(cdf.shape[0], u.shape[-1]).contiguous()
    inds = torch.searchsorted(cdf, u, side="right")
    below = torch.clamp(inds - 1, 0, b.shape[-1] - 1)
    above = torch.clamp(inds, 0, b.shape[-1] - 1)
    c0, b0 = torch.gather(cdf, -1, below), torch.gather(b, -1, below)
    c1, b1 = torch.gather(cdf, -1, above), torch.gather(b, -1, above)
    t = torch.clip(torch.nan_to_num((u - c0) / (c1 - c0), 0), 0, 1)
    return b0 + t * (b1 - b0), inds, cdf


def samples(ebins, origins, directions, dtype=torch.float32):
    """Euclidean bins [R,M+1] -> deltas [R,M], positions [R,M,3], q [R,M,3], selector [R,M] (the contraction case)."""
    e = ebins.to(dtype)
    starts, ends = e[:, :-1, None], e[:, 1:, None]
    deltas = (ends - starts)[..., 0]
    positions = onf.sample_positions(origins.to(dtype), directions.to(dtype), starts, ends)
    q, selector = onf.normalized_positions(positions)
    return deltas, positions, q, selector


# ---- the test inputs -------------------------------------------------------------------------------------------------------------------------
def rays(R: int, seed: int = 0, far_out: bool = False):
    """origins around the unit box, unit directions, per-ray nears in [0.02, 0.3] and fars in [2, 60].  far_out (the uniform sampler's
    rays that miss a render box): every 11th ray ends at 1e10, where the contraction lands on the face q = 1 and the selector drops it."""
    g = torch.Generator().manual_seed(1000 + seed)
    o = torch.rand(R, 3, generator=g) * 2.4 - 1.2
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    nears = 0.02 + 0.28 * torch.rand(R, generator=g)
    fars = 2.0 + 58.0 * torch.rand(R, generator=g)
    if far_out:
        fars[3::11] = 1e10
    return o, d, nears, fars


def uniforms(R: int, n_edges: int, single_jitter: bool, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.rand(R, generator=g) if single_jitter else torch.rand(R, n_edges, generator=g)


def weights(R: int, N: int, seed: int = 0) -> torch.Tensor:
    """rand^8 (a few samples carry a ray), a fifth of the rays all-zero, a few one-hot rows."""
    g = torch.Generator().manual_seed(3000 + seed)
    w = torch.rand(R, N, generator=g) ** 8
    w[::5] = 0.0
    for r in range(2, R, 7):
        w[r] = 0.0
        w[r, (r * 13) % N] = 1.0
    return w


def previous_level(R: int, N: int, seed: int = 0):
    """The level a resampling step starts from: jittered spacing bins of N intervals and weights."""
    base = torch.linspace(0.0, 1.0, N + 1)
    return initial_bins(base, uniforms(R, N + 1, False, seed + 17)), weights(R, N, seed)


def decreasing_pairs(bins: torch.Tensor) -> int:
    return int((bins[:, 1:] < bins[:, :-1]).sum())
