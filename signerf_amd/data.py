"""The data half of training: pixel samplers, ``RayGenerator`` and an in-process ``SIGNeRFDataManager`` -- (camera, y, x) triplets in, a
flat ``RayBundle`` and the matching target pixels out, in ONE launch of the HIP library (``sn_generate_ray_batch``).

What the reference runs (signerf/data/signerf_datamanager.py): nerfstudio's ``DataProcessor`` workers sample ``ray_indices`` with a
``PixelSampler`` (``PatchPixelSampler`` of signerf/data/signerf_patch_pixel_sampler.py when ``patch_size > 1``, :124-129), gather the pixels
on the CPU, and turn the indices into rays with ``RayGenerator`` -> ``cameras.generate_rays(camera_indices=c[:, None], coords=...)``;
``next_train`` takes the pair off a queue and moves it to the GPU.  Here cameras and the uint8 image stack live on the GPU: the indices are
sampled there with torch ops, and one kernel writes rays and pixels.  Names and argument order are nerfstudio's.

Not here: training-mode sampling and the field's gradients (the losses and the compositing backward ARE built: signerf_amd/losses.py, the
back half of a step); per-ray distortion deltas and pose refinement; the multi-process ``DataProcessor``; eval dataloaders (the reference's own are ``TODO: Implement``); eroded-mask and equirectangular-weighted samplers.
"""

from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, Optional, Tuple, Type, Union

import torch
from torch import Tensor

from .cameras import _H_H, _H_W, Cameras, RayBundle, SceneBox


class RayGenerator:
    """nerfstudio's ``RayGenerator``: ``ray_indices`` [N, 3] = (camera, y, x) -> the ``RayBundle`` of the rays through those pixels'
    centres.  With an ``images`` stack (uint8 [B, H, W, C] on the cameras' device) given at construction the call returns
    ``(bundle, pixels)``, ``pixels`` [N, C] = ``images[c, y, x] / 255`` from the same launch.  ``aabb_box`` (extension): the bundle carries
    nears / fars of that box, as ``generate_rays(aabb_box=...)`` gives them."""

    def __init__(self, cameras: Cameras, images: Optional[Tensor] = None, aabb_box: Optional[SceneBox] = None):
        self.cameras = cameras
        self.images = images
        self.aabb_box = aabb_box

    def __call__(self, ray_indices: Tensor):
        bundle, pixels = self.cameras.generate_rays_from_indices(ray_indices, images=self.images, aabb_box=self.aabb_box)
        return bundle if self.images is None else (bundle, pixels)

    forward = __call__


@dataclass
class PixelSamplerConfig:
    """nerfstudio's ``PixelSamplerConfig`` as far as the reference's datamanager reads it."""

    _target: Type = field(default_factory=lambda: PixelSampler)
    num_rays_per_batch: int = 4096
    """number of rays to sample per batch"""
    keep_full_image: bool = False
    """whether ``sample`` also returns the whole image stack (``full_image``)"""
    ignore_mask: bool = False
    """sample everywhere even where the batch has a mask"""

    def setup(self, **kwargs):
        return self._target(self, **kwargs)


class PixelSampler:
    """nerfstudio's ``PixelSampler``: uniform (image, y, x) indices.  ``generator`` (extension): the ``torch.Generator`` the random numbers
    come from -- it must live on the device that is sampled on; None = the global RNG."""

    config: PixelSamplerConfig

    def __init__(self, config: PixelSamplerConfig, generator: Optional[torch.Generator] = None, **kwargs) -> None:
        names = {f.name for f in dataclasses.fields(config)} - {"_target"}
        unknown = set(kwargs) - names
        if unknown:
            raise TypeError(f"{type(config).__name__} has no field {', '.join(sorted(unknown))}")
        self.config = dataclasses.replace(config, **kwargs)   # (nerfstudio writes the keyword overrides into the config it was given)
        self.generator = generator
        self._consts: Dict[tuple, Tensor] = {}
        self.set_num_rays_per_batch(self.config.num_rays_per_batch)

    def set_num_rays_per_batch(self, num_rays_per_batch: int):
        self.num_rays_per_batch = num_rays_per_batch

    def _const(self, values, device) -> Tensor:
        """A small constant tensor on ``device``, uploaded once: sampling must not copy from the host on every step."""
        key = (tuple(values), str(device))
        t = self._consts.get(key)
        if t is None:
            t = self._consts[key] = torch.tensor(values, dtype=torch.float32, device=device)
        return t

    def sample_method(self, batch_size: int, num_images: int, image_height: int, image_width: int, mask: Optional[Tensor] = None,
                      device: Union[torch.device, str] = "cpu") -> Tensor:
        """int64 [batch_size, 3] (image, y, x).  Without a mask ``floor(rand(batch_size, 3) * [num_images, H, W])``; with a mask
        [B, H, W, 1] a uniform choice (with replacement) among ``nonzero(mask[..., 0])`` -- that one waits for the device, as ``nonzero``
        does."""
        if isinstance(mask, Tensor) and not self.config.ignore_mask:
            nonzero_indices = torch.nonzero(mask[..., 0].to(device), as_tuple=False)
            if nonzero_indices.shape[0] == 0:
                raise ValueError("the mask selects no pixel")
            chosen = torch.floor(torch.rand((batch_size,), device=device, generator=self.generator) * nonzero_indices.shape[0]).long()
            return nonzero_indices[chosen.clamp_(max=nonzero_indices.shape[0] - 1)]
        scale = self._const((num_images, image_height, image_width), device)
        return torch.floor(torch.rand((batch_size, 3), device=device, generator=self.generator) * scale).long()

    def sample(self, image_batch: Dict) -> Dict:
        """nerfstudio's ``collate_image_dataset_batch``: ``image_batch`` holds ``image`` [B, H, W, C], ``image_idx`` [B] and optionally
        ``mask`` [B, H, W, 1]; returns ``indices`` [N, 3] (camera = ``image_idx`` of the sampled image, y, x) and every per-pixel entry
        gathered at them (a uint8 ``image`` as fp32 / 255)."""
        image = image_batch["image"]
        if not isinstance(image, Tensor):
            raise NotImplementedError("a list of images (variable resolution) is not supported: the images must have one size")
        device = image.device
        num_images, image_height, image_width, _ = image.shape
        indices = self.sample_method(self.num_rays_per_batch, num_images, image_height, image_width, mask=image_batch.get("mask"), device=device)
        c, y, x = (i.flatten() for i in torch.split(indices, 1, dim=-1))
        out = {}
        for key, value in image_batch.items():
            if key != "image_idx" and isinstance(value, Tensor) and value.ndim >= 3 and tuple(value.shape[:3]) == tuple(image.shape[:3]):
                v = value[c.to(value.device), y.to(value.device), x.to(value.device)]
                out[key] = v.float() / 255 if v.dtype == torch.uint8 and key == "image" else v
        indices = indices.clone()
        indices[:, 0] = image_batch["image_idx"].to(device)[c]
        out["indices"] = indices
        if self.config.keep_full_image:
            out["full_image"] = image
        return out


@dataclass
class PatchPixelSamplerConfig(PixelSamplerConfig):
    """signerf/data/signerf_patch_pixel_sampler.py::PatchPixelSamplerConfig."""

    _target: Type = field(default_factory=lambda: PatchPixelSampler)
    patch_size: int = 32
    """side length of a patch; must agree with the method config's ``patch_size`` for the batch to reshape into patches"""


class PatchPixelSampler(PixelSampler):
    """signerf/data/signerf_patch_pixel_sampler.py::PatchPixelSampler: square patches at random positions of random images, flattened
    patch by patch -- ``patch_size ** 2`` consecutive rays are one patch of one image."""

    config: PatchPixelSamplerConfig

    def set_num_rays_per_batch(self, num_rays_per_batch: int):
        self.num_rays_per_batch = (num_rays_per_batch // (self.config.patch_size**2)) * (self.config.patch_size**2)

    def sample_method(self, batch_size: int, num_images: int, image_height: int, image_width: int, mask: Optional[Tensor] = None,
                      device: Union[torch.device, str] = "cpu") -> Tensor:
        if isinstance(mask, Tensor) and not self.config.ignore_mask:
            # with a mask the reference's sampler reduces to the base one (its eroded-mask sampling is removed there)
            return super().sample_method(batch_size, num_images, image_height, image_width, mask=mask, device=device)
        ps = self.config.patch_size
        if image_height < ps or image_width < ps:
            raise ValueError(f"patch_size {ps} does not fit a {image_height} x {image_width} image")
        sub_bs = batch_size // (ps**2)
        scale = self._const((num_images, image_height - ps, image_width - ps), device)
        origins = torch.rand((sub_bs, 3), device=device, generator=self.generator) * scale
        key = ("grid", ps, str(device))
        grid = self._consts.get(key)
        if grid is None:   # [ps, ps, 3] = (0, yy, xx)
            yys, xxs = torch.meshgrid(torch.arange(ps, device=device), torch.arange(ps, device=device), indexing="ij")
            grid = self._consts[key] = torch.stack([torch.zeros_like(yys), yys, xxs], dim=-1).to(torch.float32)
        indices = origins.view(sub_bs, 1, 1, 3) + grid
        return torch.floor(indices).long().flatten(0, 2)


@dataclass
class SIGNeRFDataManagerConfig:
    """The fields of the reference's ``SIGNeRFDataManagerConfig`` (nerfstudio's ``VanillaDataManagerConfig``) that ``next_train`` depends
    on; the worker and queue settings have no counterpart here."""

    _target: Type = field(default_factory=lambda: SIGNeRFDataManager)
    train_num_rays_per_batch: int = 4096
    patch_size: int = 1
    """> 1: patches of this side length (``PatchPixelSampler``)"""
    pixel_sampler: PixelSamplerConfig = field(default_factory=PixelSamplerConfig)


class SIGNeRFDataManager:
    """In-process stand-in for signerf/data/signerf_datamanager.py::SIGNeRFDataManager's training side, built from a ``Cameras`` and a
    uint8 image stack [B, H, W, C] on the GPU (one image per camera, all of one size).  ``next_train`` samples indices with torch ops on
    the GPU and issues one library launch for rays and pixels; it does not wait for the device.  No worker processes, no queue."""

    def __init__(self, config: Optional[SIGNeRFDataManagerConfig], cameras: Cameras, images: Tensor, masks: Optional[Tensor] = None,
                 aabb_box: Optional[SceneBox] = None, generator: Optional[torch.Generator] = None):
        self.config = config if config is not None else SIGNeRFDataManagerConfig()
        if cameras.device.type != "cuda":
            raise ValueError("SIGNeRFDataManager needs the cameras on the GPU: call .to('cuda') first")
        if not isinstance(images, Tensor) or images.dtype != torch.uint8 or images.ndim != 4 or images.shape[0] != cameras.size:
            raise ValueError(f"images must be one uint8 stack [{cameras.size}, H, W, C]: an image per camera, all of one size")
        sizes = {(int(h), int(w)) for h, w in zip(cameras._host[:, _H_H].tolist(), cameras._host[:, _H_W].tolist())}
        if sizes != {(images.shape[1], images.shape[2])}:
            raise NotImplementedError(f"variable resolution is not supported: the cameras are {sorted(sizes)} (height, width), the image "
                                      f"stack is {tuple(images.shape[1:3])}; every camera must have the stack's size")
        self.device = cameras.device
        self.train_cameras = cameras
        self.images = images.to(self.device).contiguous()
        self.masks = None if masks is None else masks.to(self.device)
        self.train_count = 0
        self.train_pixel_sampler = self._get_pixel_sampler(self.config.train_num_rays_per_batch, generator)
        self.train_ray_generator = RayGenerator(cameras, images=self.images, aabb_box=aabb_box)

    @classmethod
    def from_directory(cls, path: Union[str, Path], config: Optional[SIGNeRFDataManagerConfig] = None, device: Union[torch.device, str] = "cuda",
                       aabb_box: Optional[SceneBox] = None, generator: Optional[torch.Generator] = None) -> "SIGNeRFDataManager":
        """From a dataset directory as ``generate_dataset`` writes it: ``transforms.json`` (per-frame intrinsics and poses) and the images
        its frames name."""
        import numpy as np
        from PIL import Image

        from .dataset_io import load_generated_frames

        fr = load_generated_frames(Path(path) / "transforms.json")
        arrays = []
        for p in fr["file_paths"]:
            with Image.open(p) as im:
                arrays.append(np.asarray(im.convert("RGB") if im.mode not in ("RGB", "L") else im, dtype=np.uint8))
        shapes = sorted({a.shape for a in arrays})
        if len(shapes) != 1:
            raise NotImplementedError(f"variable resolution is not supported: the images of {path} have the sizes {shapes}")
        stack = torch.from_numpy(np.stack(arrays))
        if stack.ndim == 3:
            stack = stack[..., None]
        cameras = Cameras(fr["camera_to_worlds"], fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["width"], fr["height"]).to(device)
        return cls(config, cameras, stack.to(device), aabb_box=aabb_box, generator=generator)

    def _get_pixel_sampler(self, num_rays_per_batch: int, generator: Optional[torch.Generator] = None) -> PixelSampler:
        """signerf_datamanager.py:124-129: patches when ``patch_size > 1`` and the configured sampler is the plain one."""
        if self.config.patch_size > 1 and type(self.config.pixel_sampler) is PixelSamplerConfig:
            return PatchPixelSamplerConfig().setup(patch_size=self.config.patch_size, num_rays_per_batch=num_rays_per_batch, generator=generator)
        return self.config.pixel_sampler.setup(num_rays_per_batch=num_rays_per_batch, generator=generator)

    def next_train(self, step: int) -> Tuple[RayBundle, Dict]:
        """(RayBundle [N], batch): ``batch["indices"]`` int64 [N, 3] (camera, y, x) and ``batch["image"]`` fp32 [N, C], the target pixels."""
        self.train_count += 1
        b, h, w, _ = self.images.shape
        sampler = self.train_pixel_sampler
        indices = sampler.sample_method(sampler.num_rays_per_batch, b, h, w, mask=self.masks, device=self.device)
        ray_bundle, pixels = self.train_ray_generator(indices)
        return ray_bundle, {"indices": indices, "image": pixels}

    def get_train_rays_per_batch(self) -> int:
        if self.train_pixel_sampler is not None:
            return self.train_pixel_sampler.num_rays_per_batch
        return self.config.train_num_rays_per_batch
