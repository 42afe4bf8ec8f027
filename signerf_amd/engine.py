"""``Engine`` -- the eval-mode HIP handle of one ``NerfactoModel``: its lifecycle, its locking and the render calls on it.

The model's parameters live in ``nn.Module``s under nerfstudio's state-dict names; the eval render reads a copy of them inside a handle of
the C ABI (``sn_create`` ... ``sn_destroy``).  The engine creates the handle on the model's device, uploads the parameters when they are
dirty, starts over when the model moved or ``precision="fp16"`` asks for grid storage the handle lacks, and destroys it with the model.  The
ABI orders uploads against renders ON THE DEVICE, but the host-side sequence sn_upload_weights ... sn_finalize_weights leaves the handle
un-finalized in between, so no call on the handle may start inside it, or while the handle is replaced.  One spelling enforces that:

    engine.ensure()                              # (the write lock, when there is something to do)
    with engine.reading() as (lib, handle):      # (the read lock)
        lib.sn_...(handle, ...)

``reading()`` is never nested -- writers have preference, so a reader that re-enters while an upload waits would deadlock: a function takes
it in its outermost frame, and what it calls inside (``opts``) does not take it again.  ``ensure()`` comes before ``reading()``, never inside."""

from __future__ import annotations

import contextlib
import ctypes as C
import threading
import warnings
import weakref
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib

PRECISIONS = {"fp32": 0, "fp16x2": 1, "fp16": 2}   # "fp16": opt-in, implementation="tcnn" only (config.py)
# RGBRenderer's background in EVAL mode [NS]: "last_sample" (nerfacto's default, what SIGNeRF runs), a named constant colour, or "random" --
# a training device: combine_rgb returns the composited colour without a background, i.e. black
BACKGROUNDS = {"last_sample": None, "black": (0.0, 0.0, 0.0), "white": (1.0, 1.0, 1.0), "random": (0.0, 0.0, 0.0)}
# NerfactoModelConfig.proposal_initial_sampler [NS] -> SnRenderOpts.spacing_mode: UniformLinDispPiecewiseSampler (the default) or UniformSampler
INITIAL_SAMPLERS = {"piecewise": 0, "uniform": 1}


class _RWLock:
    """Many calls on the handle, or one weight upload.  Writers have preference: a waiting upload blocks NEW readers, so a viewer that
    renders back to back on the shared model cannot starve the generator thread's reload."""

    def __init__(self):
        self._cond = threading.Condition()
        self._readers = 0
        self._writer = False
        self._writers_waiting = 0

    def acquire_read(self):
        with self._cond:
            while self._writer or self._writers_waiting:
                self._cond.wait()
            self._readers += 1

    def release_read(self):
        with self._cond:
            self._readers -= 1
            if self._readers == 0:
                self._cond.notify_all()

    def acquire_write(self):
        with self._cond:
            self._writers_waiting += 1
            try:
                while self._writer or self._readers:
                    self._cond.wait()
            finally:
                self._writers_waiting -= 1
            self._writer = True

    def release_write(self):
        with self._cond:
            self._writer = False
            self._cond.notify_all()


def wants_half_grid(cfg) -> bool:
    """The single-fp16 mode keeps the tiny-cuda-nn grid in fp16 storage as well (half the gather bytes; include/signerf_hip.h half_grid)."""
    return cfg.precision == "fp16" and cfg.implementation == "tcnn"


def lifecycle(has_handle: bool, device_moved: bool, dirty: bool, want_half: bool, has_half: bool) -> Tuple[bool, bool, bool]:
    """What ``ensure()`` has to do -> (destroy, create, upload).  A handle on another device than the model's, or one created without the
    grid's fp16 storage that ``precision="fp16"`` now wants, is started over; a new handle is empty, so it is always uploaded to."""
    destroy = has_handle and (device_moved or (want_half and not has_half))
    create = destroy or not has_handle
    return destroy, create, create or dirty


def _f32_on(dev, t: Optional[Tensor]) -> Optional[Tensor]:
    return None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()


class Engine:
    """A plain object in the model's ``__dict__`` (no sub-module, not in the state dict) that holds the model weakly: the model's refcount
    alone decides when the handle, and the device memory behind it, is released."""

    def __init__(self, owner):
        self._owner = weakref.ref(owner)
        self._lib = None                   # the library that made the handle: set by ensure()
        self.handle = C.c_void_p(None)
        self.generation = 0                # bumped whenever the handle's weights are (re)written
        self.dirty = True
        self.march_stats: Optional[Tensor] = None   # diagnostics (ops.render_with_march_stats): 3 uint64 counters the kernels add to
        self._device = None
        self._half_grid = False            # whether the handle holds the grid's fp16 storage (SnFieldDesc.half_grid)
        self._upload_lock = threading.Lock()
        self._rw = _RWLock()
        self._grid_cache: Dict = {}
        self._fallback_warned = False

    @contextlib.contextmanager
    def reading(self):
        """The read lock around calls on the handle -> (lib, handle); both None / NULL before the first ``ensure()``."""
        self._rw.acquire_read()
        try:
            yield self._lib, self.handle
        finally:
            self._rw.release_read()

    def effective_precision(self, kernel: int = 0) -> str:
        """What ``config.precision`` resolves to for the uploaded parameters ("fp16x2" falls back to "fp32" for a handle whose split-
        precision MLPs cannot be range-conditioned; sn_effective_precision).  kernel 0: render / field kernels, 1: normals."""
        want = self._owner().config.precision
        with self.reading() as (lib, handle):
            if not handle or self.dirty:
                return want
            eff = lib.sn_effective_precision(handle, PRECISIONS[want], kernel)
        return {0: "fp32", 1: "fp16x2", 2: "fp16"}.get(eff, want)

    def ensure(self):
        """A finalized handle on the model's device that holds the model's current parameters -> lib."""
        lib = self._lib = _lib.load()
        model = self._owner()
        cfg, dev = model.config, model.device
        if dev.type != "cuda":
            raise _lib.SignerfHipError("NerfactoModel renders on the GPU only: move it with .to('cuda') (no CPU fallback)")
        with self._upload_lock:
            destroy, create, upload = lifecycle(bool(self.handle), self._device != dev, self.dirty, wants_half_grid(cfg), self._half_grid)
            if upload:
                # the handle is replaced / its weights rewritten: no CALL of another thread may hold or take the handle meanwhile
                self._rw.acquire_write()
                try:
                    if destroy:   # e.g. model.to("cuda:N") after the first render: the handle and all its buffers live on the old GPU
                        self.close()
                    if create:
                        desc = model._field_desc()
                        with torch.cuda.device(dev):
                            _lib.check(lib.sn_create(C.byref(desc), C.byref(self.handle)), None, "sn_create")
                        self._device = dev
                        self._half_grid = bool(desc.half_grid)
                    self._upload(lib, model)
                    self.dirty = False
                    self.generation += 1   # (a kept render state of the old weights no longer matches: render_normals)
                finally:
                    self._rw.release_write()
        if not self._fallback_warned and self.effective_precision() != cfg.precision:
            self._fallback_warned = True
            # a wide field: only the exact-fp32 MFMA arithmetic is built (DESIGN.md §4 "Wide fields")
            why = "is not built for wide fields (hidden_dim=128)" if cfg.hidden_dim == 128 else "cannot hold fp32 grade for these parameters"
            warnings.warn(f"signerf_amd: precision={cfg.precision!r} {why}; "
                          f"rendering with {self.effective_precision()!r}", RuntimeWarning, stacklevel=3)
        return lib

    def _upload(self, lib, model):
        stream = _lib.current_stream()
        cfg = model.config

        def up(name: str, t: Tensor):
            t = t.detach().to(torch.float32).contiguous()
            buf = t if t.is_cuda else t.cpu()
            _lib.check(lib.sn_upload_weights(self.handle, name.encode(), buf.data_ptr(), buf.numel() * 4, stream),
                       self.handle, f"sn_upload_weights({name})")

        with torch.cuda.device(model.device):
            for k, v in model.state_dict().items():
                if (k.endswith("hash_table") or ".mlp.layers." in k or k.startswith("field.mlp_head.layers.")
                        or (model._has_pred_normals and k.startswith(("field.mlp_pred_normals.layers.", "field.field_head_pred_normals.net.")))):
                    up(k, v)
            if cfg.appearance_embed_dim > 0:
                if cfg.use_average_appearance_embedding:
                    app = model.field.embedding_appearance.mean(0)
                else:
                    app = torch.zeros(cfg.appearance_embed_dim, device=model.device)
                up("field.embedding_appearance.mean", app)
            _lib.check(lib.sn_finalize_weights(self.handle, stream), self.handle, "sn_finalize_weights")
            # "fp16x2" is a request: the library conditions the split-precision MLPs into fp16's range from the uploaded parameters and
            # falls back to the exact-fp32 MFMA path for a handle it cannot condition (include/signerf_hip.h, sn_effective_precision)
            self._fallback_warned = False

    def close(self):
        """Destroys the handle, once: a second call, or one before any handle was made, does nothing."""
        if self.handle:
            handle, self.handle = self.handle, C.c_void_p(None)
            self.dirty = True
            self._grid_cache.clear()
            self._lib.sn_destroy(handle)

    # sampler grids, computed with the same torch ops nerfstudio uses (bit-identical to the reference's)
    def grids(self, n_levels: int):
        model = self._owner()
        cfg, dev = model.config, model.device
        counts = list(cfg.num_proposal_samples_per_ray[:n_levels]) + [cfg.num_nerf_samples_per_ray]
        key = (tuple(counts), str(dev))
        if key not in self._grid_cache:
            bins0 = torch.linspace(0.0, 1.0, counts[0] + 1)
            us = []
            for m in counts[1:]:
                nb = m + 1
                u = torch.linspace(0.0, 1.0 - (1.0 / nb), steps=nb) + 1.0 / (2 * nb)
                us.append(u.to(dev))
            self._grid_cache[key] = (bins0.to(dev), us)
        return self._grid_cache[key]

    def opts(self, lib, handle, H: int, W: int, single_chunk: bool = False):
        """-> (SnRenderOpts of the model's config for an H x W frame, (workspace, grids): what its pointers point to).  ``lib, handle``:
        what the caller's ``reading()`` yielded -- the handle is asked for the workspace size."""
        model = self._owner()
        cfg = model.config
        n_levels = cfg.num_proposal_iterations
        o = _lib.SnRenderOpts()
        o.num_proposal_iterations = n_levels
        for i in range(n_levels):
            o.num_proposal_samples[i] = cfg.num_proposal_samples_per_ray[i]
        o.num_nerf_samples = cfg.num_nerf_samples_per_ray
        o.near_plane = cfg.near_plane if model.training else 0.0  # NearFarCollider: eval near = 0 (A3)
        o.far_plane = cfg.far_plane
        # the chunk size only shapes the expected-depth clip bounds (A17): per eval_num_rays_per_chunk rays for a camera bundle
        # (Model.get_outputs_for_camera_ray_bundle's loop), over the whole bundle for Model.get_outputs / forward
        o.chunk_rays = max(H * W, 1) if single_chunk else cfg.eval_num_rays_per_chunk
        o.precision = PRECISIONS[cfg.precision]
        bg = BACKGROUNDS[cfg.background_color]
        o.background_mode = 0 if bg is None else 1
        o.spacing_mode = INITIAL_SAMPLERS[cfg.proposal_initial_sampler]
        o.march_stats = self.march_stats.data_ptr() if self.march_stats is not None else None
        for c in range(3):
            o.background_rgb[c] = 0.0 if bg is None else bg[c]
        bins0, us = self.grids(n_levels)
        o.initial_spacing_bins = bins0.data_ptr()
        for i, u in enumerate(us):
            o.pdf_u[i] = u.data_ptr()
        need = lib.sn_workspace_bytes(handle, H, W, C.byref(o))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=model.device)
        o.workspace = ws.data_ptr()
        o.workspace_bytes = ws.numel()
        return o, (ws, bins0, us)

    def render(self, b, H: int, W: int, single_chunk: bool = False, keep_state: bool = False, keep_state_max_bytes=None):
        """-> (outputs, state).  state: what ``render_normals`` needs to re-use this render's final sample bins; None without ``keep_state``
        or for a workspace larger than ``keep_state_max_bytes`` (config.normals_bin_reuse_max_mb)."""
        self.ensure()
        model = self._owner()
        dev, nprop = model.device, model.config.num_proposal_iterations
        n = H * W
        with torch.cuda.device(dev):
            new = lambda c: torch.empty((n, c), dtype=torch.float32, device=dev)  # noqa: E731
            out = {"rgb": new(3), "accumulation": new(1), "depth": new(1), "expected_depth": new(1)}
            out.update({f"prop_depth_{i}": new(1) for i in range(nprop)})
            if n == 0:  # an empty bundle renders to empty outputs, as the reference's chunk loop does
                return out, None
            rays = tuple(_f32_on(dev, t) for t in (b.origins, b.directions, b.nears, b.fars))
            pp = [_lib.ptr(out[f"prop_depth_{i}"]) for i in range(nprop)] + [None] * (2 - nprop)
            state = None
            with self.reading() as (lib, handle):
                o, keep = self.opts(lib, handle, H, W, single_chunk)
                st = lib.sn_render_rays(handle, *map(_lib.ptr, rays), H, W, C.byref(o), _lib.ptr(out["rgb"]), _lib.ptr(out["depth"]),
                                        _lib.ptr(out["accumulation"]), _lib.ptr(out["expected_depth"]), pp[0], pp[1], _lib.current_stream())
                _lib.check(st, handle, "sn_render_rays")
                if keep_state and (keep_state_max_bytes is None or keep[0].numel() <= keep_state_max_bytes):
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(dev))
                    state = {"opts": o, "keep": keep, "rays": rays, "event": ev, "generation": self.generation}
            # (the workspace and grids in `keep` are consumed by work already enqueued on this stream; the caching allocator is
            # stream-ordered, so letting them go when this frame returns is safe)
        return out, state

    def render_normals(self, b, H: int, W: int, state=None) -> Dict[str, Tensor]:
        """Row a16: "normals" (analytic) and "pred_normals", [H*W,3] each, by the separate normals kernel (csrc/sn_normals.h).
        ``state`` = what ``render(..., keep_state=True)`` kept of the colour render of the SAME bundle: its options, its workspace
        (the final sample bins are still in it) and an event behind its kernels -- the proposal sampler is then not run again."""
        self.ensure()
        model = self._owner()
        dev = model.device
        with torch.cuda.device(dev):
            out = {"normals": torch.empty((H * W, 3), dtype=torch.float32, device=dev)}
            if model._has_pred_normals:
                out["pred_normals"] = torch.empty((H * W, 3), dtype=torch.float32, device=dev)
            if H * W == 0:
                return out
            reuse = state is not None and state["generation"] == self.generation
            # the very tensors the colour render marched (the library's workspace stamp compares their addresses: a second fp32 / contiguous
            # copy of a bundle that needed one would be "another bundle")
            rays = state["rays"] if reuse else tuple(_f32_on(dev, t) for t in (b.origins, b.directions, b.nears, b.fars))
            with self.reading() as (lib, handle):
                while True:
                    if reuse:
                        o, keep = state["opts"], state["keep"]
                        o.reuse_final_bins = 1
                        cur = torch.cuda.current_stream(dev)
                        cur.wait_event(state["event"])            # (a viewer thread may read the normals on another stream)
                        keep[0].record_stream(cur)
                    else:
                        o, keep = self.opts(lib, handle, H, W)
                    o.march_stats = None   # (the colour render of this frame has counted the proposal levels already)
                    st = lib.sn_render_normals(handle, *map(_lib.ptr, rays), H, W, C.byref(o), _lib.ptr(out["normals"]),
                                               _lib.ptr(out.get("pred_normals")), _lib.current_stream())
                    if not (reuse and st == _lib.SN_ERR_STATE):
                        break
                    # the library found that the workspace no longer holds this frame's bins (weights re-uploaded in between, the
                    # memory handed to another call): not an error for the caller -- the proposal kernel runs again
                    msg = lib.sn_last_error(handle)
                    warnings.warn("lazy normals: the kept sample bins could not be re-used (%s); running the proposal sampler again"
                                  % (msg.decode() if msg else ""), RuntimeWarning)
                    reuse = False
                _lib.check(st, handle, "sn_render_normals")
        return out
