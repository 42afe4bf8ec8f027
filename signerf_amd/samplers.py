"""Training-mode proposal sampling in HIP (include/signerf_hip_sampler.h, csrc/sn_sampler.h) behind nerfstudio's names and shapes
[NS-RECALL, nerfstudio 1.0.2 ``model_components/ray_samplers.py``]: ``SpacedSampler`` and ``PDFSampler`` in their training branch
(stratified jitter, ``include_original=False``) as ``sample_initial`` / ``sample_pdf``, and ``ProposalNetworkSampler``, which produces the
``ray_samples_list`` / ``weights_list`` that ``NerfactoModel.get_loss_dict`` reads (DESIGN.md §4 "Training-mode sampling").

Inputs are fp32 GPU tensors: another dtype raises ``TypeError``, a CPU tensor raises ``SignerfHipError`` (there is no CPU path), a
non-contiguous tensor is made contiguous.  Nothing here gets a gradient: nerfstudio detaches the bins, and the weights a resampling step
reads are detached as well.  A returned ``RaySamples`` carries, beside nerfstudio's members, two attributes the kernels fill in the same
pass: ``q`` [R,S,3], the field's normalised positions (scene contraction, (p + 2) / 4, multiplied by the selector), and ``selector``
[R,S] (bool) -- ``oracle.nerfacto.normalized_positions``; with ``disable_scene_contraction`` the fields normalise with torch ops instead.
(The kernels' undivided rows ride along as well, for the next resampling step and for tests: ``spacing_bins`` / ``euclid_bins`` [R,S+1],
of which ``spacing_starts`` / ``spacing_ends`` and the frustums' ``starts`` / ``ends`` are views, and ``positions`` [R,S,3].)

Random numbers: with ``rand=None`` the kernels draw from Philox4x32-10 under (``seed``, ``offset``); no two launches of a run may share
an (seed, offset) pair -- ``ProposalNetworkSampler`` hands out ``4 * call + level``.  ``rand`` (a tensor [R] under single jitter, else
[R, S+1]) replaces the generator; ``return_rand=True`` also returns the numbers that were used.
"""

from __future__ import annotations

import ctypes as C
import math
from typing import Callable, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib
from .cameras import Frustums, RayBundle, RaySamples

MAX_SAMPLES = 1024
SPACING_MODES = {"piecewise": 0, "uniform": 1}
TAKES = "the sampler kernels take fp32 rays, bins and weights"
_GRIDS: dict = {}   # (kind, n, device) -> the uploaded linspace


def _count(n, what: str) -> int:
    if not isinstance(n, int) or not 1 <= n <= MAX_SAMPLES:
        raise ValueError(f"{what}: 1..{MAX_SAMPLES} samples per ray expected, got {n!r}")
    return n


def _grid(kind: str, n: int, device) -> Tensor:
    """The base bins linspace(0, 1, n+1) of the initial sampler, or the u grid linspace(0, 1 - 1/(n+1), n+1) of a resampling step: formed
    by torch on the host, as the eval path forms ``initial_spacing_bins`` / ``pdf_u``, and uploaded once per device."""
    key = (kind, n, str(device))
    if key not in _GRIDS:
        g = torch.linspace(0.0, 1.0, n + 1) if kind == "base" else torch.linspace(0.0, 1.0 - (1.0 / (n + 1)), steps=n + 1)
        _GRIDS[key] = g.to(device)
    return _GRIDS[key]


class _Rays:
    """The flattened bundle as the kernels take it."""

    def __init__(self, ray_bundle: RayBundle, near_plane: float, far_plane: float):
        b = ray_bundle
        for x, name in ((b.origins, "origins"), (b.directions, "directions")):   # every dtype before any device
            if not isinstance(x, Tensor):
                raise TypeError(f"ray_bundle.{name}: a torch.Tensor expected, got {type(x).__name__}")
            if x.dtype != torch.float32:
                raise TypeError(f"ray_bundle.{name}: fp32 expected, got {x.dtype}")
        self.shape = tuple(b.origins.shape[:-1])
        self.origins = _lib.prep(b.origins, "ray_bundle.origins", TAKES).detach().reshape(-1, 3)
        self.directions = _lib.prep(b.directions, "ray_bundle.directions", TAKES).detach().reshape(-1, 3)
        self.R = self.origins.shape[0]
        if self.directions.shape[0] != self.R:
            raise ValueError("ray_bundle: origins and directions of one shape expected")
        self.device = self.origins.device
        # a bundle without nears / fars: the collider's planes (NearFarCollider while training: near = near_plane)
        self.nears = None if b.nears is None else _lib.prep(b.nears, "ray_bundle.nears", TAKES).detach().reshape(-1)
        self.fars = None if b.fars is None else _lib.prep(b.fars, "ray_bundle.fars", TAKES).detach().reshape(-1)
        for t, name in ((self.nears, "nears"), (self.fars, "fars")):
            if t is not None and t.numel() != self.R:
                raise ValueError(f"ray_bundle.{name}: one value per ray expected")
        self.near_plane, self.far_plane = float(near_plane), float(far_plane)
        self.pixel_area = None if b.pixel_area is None else b.pixel_area.reshape(-1, 1)
        self.camera_indices = None if b.camera_indices is None else b.camera_indices.reshape(-1, 1)


def _launch(rays: _Rays, S: int, spacing_mode: str, single_jitter: bool, rand: Optional[Tensor], seed: int, offset: int, return_rand: bool,
            pdf: Optional[Tuple[Tensor, Tensor, float, float]]):
    if spacing_mode not in SPACING_MODES:
        raise ValueError(f"spacing_mode={spacing_mode!r}: one of {sorted(SPACING_MODES)} expected")
    R, dev = rays.R, rays.device
    if rand is not None:
        rand = _lib.prep(rand, "rand", TAKES).detach()
        want = (R,) if single_jitter else (R, S + 1)
        if rand.numel() != math.prod(want) or rand.device != dev:
            raise ValueError(f"rand: a tensor {list(want)} on {dev} expected, got {tuple(rand.shape)} on {rand.device}")
        rand = rand.reshape(want)
    with torch.cuda.device(dev):
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        sbins, ebins, deltas, pos, q = f(R, S + 1), f(R, S + 1), f(R, S), f(R, S, 3), f(R, S, 3)
        sel = torch.empty((R, S), dtype=torch.uint8, device=dev)
        rand_out = (f(R) if single_jitter else f(R, S + 1)) if return_rand else None
        if R > 0:
            a = _lib.SnSamplerRays()
            a.n_samples, a.n_rays = S, R
            a.origins, a.directions, a.nears, a.fars = _lib.ptr(rays.origins), _lib.ptr(rays.directions), _lib.ptr(rays.nears), _lib.ptr(rays.fars)
            a.near_plane, a.far_plane = rays.near_plane, rays.far_plane
            a.spacing_mode, a.single_jitter = SPACING_MODES[spacing_mode], 1 if single_jitter else 0
            a.rand, a.seed, a.offset = _lib.ptr(rand), seed & (2**64 - 1), offset & (2**64 - 1)
            a.spacing_bins, a.euclid_bins, a.deltas, a.positions = _lib.ptr(sbins), _lib.ptr(ebins), _lib.ptr(deltas), _lib.ptr(pos)
            a.q, a.selector, a.rand_out = _lib.ptr(q), sel.data_ptr(), _lib.ptr(rand_out)
            lib = _lib.load()
            if pdf is None:
                _lib.check(lib.sn_sampler_initial(C.byref(a), _lib.ptr(_grid("base", S, dev)), _lib.current_stream()), None, "sn_sampler_initial")
            else:
                prev_bins, weights, anneal, padding = pdf
                p = _lib.SnSamplerPdf()
                p.n_in = weights.shape[1]
                p.spacing_bins, p.weights, p.u_grid = _lib.ptr(prev_bins), _lib.ptr(weights), _lib.ptr(_grid("u", S, dev))
                p.anneal, p.histogram_padding = anneal, padding
                _lib.check(lib.sn_sampler_pdf(C.byref(a), C.byref(p), _lib.current_stream()), None, "sn_sampler_pdf")
    lead = rays.shape
    v = lambda t, c: t.reshape(*lead, S, c)  # noqa: E731
    fr = Frustums(origins=rays.origins[:, None, :].expand(R, S, 3).reshape(*lead, S, 3),
                  directions=rays.directions[:, None, :].expand(R, S, 3).reshape(*lead, S, 3),
                  starts=v(ebins[:, :-1], 1), ends=v(ebins[:, 1:], 1),
                  pixel_area=None if rays.pixel_area is None else rays.pixel_area[:, None, :].expand(R, S, 1).reshape(*lead, S, 1))
    out = RaySamples(frustums=fr,
                     camera_indices=None if rays.camera_indices is None else rays.camera_indices[:, None, :].expand(R, S, 1).reshape(*lead, S, 1),
                     deltas=v(deltas, 1), spacing_starts=v(sbins[:, :-1], 1), spacing_ends=v(sbins[:, 1:], 1))
    out.q, out.selector, out.positions = v(q, 3), sel.reshape(*lead, S).bool(), v(pos, 3)
    out.spacing_bins, out.euclid_bins = sbins.reshape(*lead, S + 1), ebins.reshape(*lead, S + 1)
    return (out, rand_out) if return_rand else out


def sample_initial(ray_bundle: RayBundle, num_samples: int, spacing_mode: str = "piecewise", single_jitter: bool = True,
                   near_plane: float = 0.05, far_plane: float = 1000.0, rand: Optional[Tensor] = None, seed: int = 0, offset: int = 0,
                   return_rand: bool = False):
    """``SpacedSampler`` (``UniformLinDispPiecewiseSampler`` / ``UniformSampler``), training branch: ``num_samples`` jittered bins per
    ray -> ``RaySamples`` [..., S]."""
    S = _count(num_samples, "sample_initial")
    rays = _Rays(ray_bundle, near_plane, far_plane)
    return _launch(rays, S, spacing_mode, bool(single_jitter), rand, int(seed), int(offset), return_rand, None)


def sample_pdf(ray_bundle: RayBundle, ray_samples: RaySamples, weights: Tensor, num_samples: int, anneal: float = 1.0,
               histogram_padding: float = 0.01, spacing_mode: str = "piecewise", single_jitter: bool = True, near_plane: float = 0.05,
               far_plane: float = 1000.0, rand: Optional[Tensor] = None, seed: int = 0, offset: int = 0, return_rand: bool = False):
    """``PDFSampler``, training branch, ``include_original=False``: resamples ``num_samples`` bins per ray from the histogram
    (``ray_samples``' spacing bins, ``pow(weights, anneal)`` [..., N, 1]) -> ``RaySamples`` [..., S]."""
    S = _count(num_samples, "sample_pdf")
    anneal = float(anneal)
    if not (anneal >= 0.0) or not math.isfinite(anneal):
        raise ValueError(f"sample_pdf: anneal must be finite and >= 0, got {anneal!r}")
    rays = _Rays(ray_bundle, near_plane, far_plane)
    weights = _lib.prep(weights, "weights", TAKES).detach()
    if ray_samples.spacing_starts is None or ray_samples.spacing_ends is None:
        raise ValueError("sample_pdf: the ray samples carry no spacing_starts / spacing_ends")
    if weights.ndim < 2 or weights.shape[-1] != 1:
        raise ValueError(f"sample_pdf: weights [..., N, 1] expected, got {tuple(weights.shape)}")
    N = _count(int(weights.shape[-2]), "sample_pdf (the previous level)")
    weights = weights.reshape(-1, N)
    prev = getattr(ray_samples, "spacing_bins", None)
    if prev is None:
        prev = torch.cat([ray_samples.spacing_starts[..., 0], ray_samples.spacing_ends[..., -1:, 0]], dim=-1)
    prev = _lib.prep(prev, "ray_samples.spacing_starts", TAKES).detach().reshape(-1, N + 1)
    if weights.shape[0] != rays.R or prev.shape[0] != rays.R:
        raise ValueError(f"sample_pdf: weights and ray samples for {rays.R} rays expected")
    return _launch(rays, S, spacing_mode, bool(single_jitter), rand, int(seed), int(offset), return_rand,
                   (prev, weights, anneal, float(histogram_padding)))


def anneal_at(step: int, slope: float, max_num_iters: int) -> float:
    """nerfacto's proposal-weight anneal: ``bias(clip(step / N, 0, 1), slope)`` with ``bias(x, b) = b x / ((b - 1) x + 1)``."""
    x = min(max(step / max_num_iters, 0.0), 1.0)
    return slope * x / ((slope - 1.0) * x + 1.0)


def update_schedule(warmup: int, update_every: int) -> Callable[[int], float]:
    """nerfacto's ``update_sched``: ``clip(interp(step, [0, warmup], [0, update_every]), 1, update_every)``."""

    def sched(step: int) -> float:
        x = update_every * min(max(step / warmup, 0.0), 1.0) if warmup > 0 else float(update_every)
        return float(min(max(x, 1.0), float(update_every)))

    return sched


class ProposalNetworkSampler:
    """nerfstudio's ``ProposalNetworkSampler``: the initial sampler, then per proposal level a density evaluation, ``get_weights`` and a
    resampling step; the last level's samples go to the main field.  ``density_fns[i]`` is called with the level's ``RaySamples`` (they
    carry ``q`` / ``selector`` beside the frustums) and returns densities [..., S, 1]; on a step that does not update the proposal
    networks it runs under ``no_grad``."""

    def __init__(self, num_nerf_samples_per_ray: int = 48, num_proposal_samples_per_ray: Sequence[int] = (256, 96),
                 num_proposal_network_iterations: int = 2, single_jitter: bool = True, update_sched: Callable[[int], float] = lambda step: 1.0,
                 initial_sampler: str = "piecewise", histogram_padding: float = 0.01, seed: int = 0, near_plane: float = 0.05,
                 far_plane: float = 1000.0):
        self.num_nerf_samples_per_ray = _count(num_nerf_samples_per_ray, "num_nerf_samples_per_ray")
        self.num_proposal_samples_per_ray = tuple(_count(int(n), "num_proposal_samples_per_ray") for n in num_proposal_samples_per_ray)
        self.num_proposal_network_iterations = int(num_proposal_network_iterations)
        if self.num_proposal_network_iterations < 1 or len(self.num_proposal_samples_per_ray) != self.num_proposal_network_iterations:
            raise ValueError("num_proposal_samples_per_ray: one count per proposal network iterations (>= 1) expected")
        if initial_sampler not in SPACING_MODES:
            raise ValueError(f"initial_sampler={initial_sampler!r}: one of {sorted(SPACING_MODES)} expected")
        self.single_jitter, self.update_sched, self.initial_sampler = bool(single_jitter), update_sched, initial_sampler
        self.histogram_padding, self.seed = float(histogram_padding), int(seed)
        self.near_plane, self.far_plane = float(near_plane), float(far_plane)
        self._anneal = 1.0
        self._steps_since_update = 0
        self._step = 0
        self._calls = 0

    def set_anneal(self, anneal: float) -> None:
        self._anneal = float(anneal)

    def step_cb(self, step: int) -> None:
        self._step = int(step)
        self._steps_since_update += 1

    def will_update(self) -> bool:
        """Whether the next call evaluates the proposal densities with a gradient."""
        return self._steps_since_update > self.update_sched(self._step) or self._step < 10

    def mark_updated(self) -> None:
        self._steps_since_update = 0

    def __call__(self, ray_bundle: RayBundle, density_fns: List[Callable]) -> Tuple[RaySamples, List[Tensor], List[RaySamples]]:
        from . import losses

        n = self.num_proposal_network_iterations
        if len(density_fns) != n:
            raise ValueError(f"{n} density functions expected, got {len(density_fns)}")
        common = dict(spacing_mode=self.initial_sampler, single_jitter=self.single_jitter, near_plane=self.near_plane, far_plane=self.far_plane,
                      seed=self.seed)
        base = 4 * self._calls           # a fresh offset per launch: no two launches of a run share a Philox counter
        self._calls += 1
        weights_list, ray_samples_list = [], []
        updated = self.will_update()
        ray_samples, weights = None, None
        for level in range(n + 1):
            last = level == n
            S = self.num_nerf_samples_per_ray if last else self.num_proposal_samples_per_ray[level]
            if level == 0:
                ray_samples = sample_initial(ray_bundle, S, offset=base, **common)
            else:
                ray_samples = sample_pdf(ray_bundle, ray_samples, weights.detach(), S, anneal=self._anneal,
                                         histogram_padding=self.histogram_padding, offset=base + level, **common)
            if not last:
                if updated:
                    density = density_fns[level](ray_samples)
                else:
                    with torch.no_grad():
                        density = density_fns[level](ray_samples)
                weights = losses.get_weights(ray_samples.deltas, density)
                weights_list.append(weights)
                ray_samples_list.append(ray_samples)
        if updated:
            self.mark_updated()
        return ray_samples, weights_list, ray_samples_list
