"""Output formats of the generated dataset -- SURVEY.md §8(f) row 3.

Mirrors what the reference writes so that ``SIGNeRFDataParser`` (signerf/data/signerf_dataparser.py:99-170,210-228) reads it
unchanged:
  * ``tensor_to_image``  /root/reference/signerf/utils/image_tensor_converter.py:7-33 -- x*255 with a TRUNCATING uint8 cast
    (254.9/255 -> 254), done by a kernel; only the finished bytes cross PCIe;
  * directory layout    datasetgenerator.py:146-182 (images/ masks/ conditions/ rendered/ originals/ *_<f>/ references/);
  * transforms.json     datasetgenerator.py:286-295 (header) and :447-466 (one frame per saved view);
  * ``load_previous_experiment_cameras``  signerf/utils/load_previous_experiment_cameras.py:12-54 (the reader of the same file).
PNG encoding is on the host by default (``encode_png``: zlib on a pool of threads; "pil": the reference's literal call) or, with
``png_encoder="hip"``, on the GPU (``encode_png_hip``: include/signerf_hip_png.h), after which the file buffer (the file and its length) crosses PCIe in one copy.
"""

from __future__ import annotations

import json
import threading
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import torch
from torch import Tensor

from . import _lib


def tensor_to_uint8(tensor: Tensor) -> Tensor:
    """[H,W,C] fp32 on the GPU -> [H,W,C] uint8 on the GPU, (uint8)(x * 255) truncating."""
    lib = _lib.load()
    t = tensor.detach().to(torch.float32).contiguous()
    with torch.cuda.device(t.device):
        out = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
        _lib.check(lib.sn_tensor_to_uint8(_lib.ptr(t), t.numel(), _lib.ptr(out), _lib.current_stream()), None, "sn_tensor_to_uint8")
    return out


def tensor_to_image(tensor: Tensor):
    """image_tensor_converter.py:7-33: [H,W,3] -> RGB image, [H,W,1] -> 'L' image."""
    from PIL import Image

    assert len(tensor.shape) == 3, "Tensor must be of shape (H, W, C)"
    u8 = tensor_to_uint8(tensor).cpu().numpy()
    if tensor.shape[2] == 1:
        return Image.fromarray(u8.squeeze(), "L")
    assert tensor.shape[2] == 3, "Tensor must be of shape (H, W, 3)"
    return Image.fromarray(u8)


def image_to_tensor(image) -> Tensor:
    """image_tensor_converter.py:35-54."""
    import numpy as np

    if image.mode == "RGBA":
        image = image.convert("RGB")
    return torch.from_numpy(np.array(image, dtype="float32")) / 255.0


def load_previous_experiment_cameras(transforms_path: Union[str, Path]) -> Tuple[Tensor, Optional[Tensor], bool]:
    """load_previous_experiment_cameras.py:12-54: (reference c2w [R,3,4], synthetic c2w [S,3,4] | None, is_combined)."""
    with open(transforms_path) as f:
        transforms = json.load(f)
    frames = transforms["frames"]

    def stack(indices: List[int]) -> Tensor:
        return torch.stack([torch.tensor(frames[i]["scene_transform_matrix"][:3], dtype=torch.float32) for i in indices], dim=0)

    reference = stack(transforms["reference_indices"])
    synthetic = stack(transforms["generated_indices"]) if transforms.get("is_synthetic") else None
    return reference, synthetic, bool(transforms.get("is_combined", False))


def load_generated_frames(transforms_path: Union[str, Path]) -> Dict[str, Any]:
    """The frames of a transforms.json that ``GeneratedDataset.save_generated_images`` wrote, as the columns a ``Cameras`` is built from:
    ``camera_to_worlds`` [N,3,4] (the frames' ``transform_matrix``: scene space), ``fx, fy, cx, cy`` fp32 [N], ``width, height`` int64
    [N] and ``file_paths`` (absolute, the frames' ``file_path`` resolved against the file's directory)."""
    transforms_path = Path(transforms_path)
    with open(transforms_path) as f:
        frames = json.load(f)["frames"]
    if not frames:
        raise ValueError(f"{transforms_path} holds no frames")
    col = lambda key, dt: torch.tensor([fr[key] for fr in frames], dtype=dt)  # noqa: E731
    return {"camera_to_worlds": torch.stack([torch.tensor(fr["transform_matrix"], dtype=torch.float32)[:3] for fr in frames], dim=0),
            "fx": col("fl_x", torch.float32), "fy": col("fl_y", torch.float32), "cx": col("cx", torch.float32),
            "cy": col("cy", torch.float32), "width": col("w", torch.int64), "height": col("h", torch.int64),
            "file_paths": [transforms_path.parent / fr["file_path"] for fr in frames]}


def encode_png(u8, compress_level: int = 6) -> bytes:
    """A PNG file of an 8-bit [H,W,1] (greyscale) or [H,W,3] (RGB) array -- the same pixels `PIL.Image.save` writes, encoded WITHOUT the
    interpreter lock: numpy forms the filtered scanlines (filter "Up": each row minus the row above, row 0 unfiltered) and `zlib.compress`
    deflates them, both of which release the GIL, so a pool of host threads really encodes in parallel (Pillow's encoder holds the lock:
    measured r04, 16 / 32 / 64 / 96 threads all took 1.4 s for config 5's 470 files).  Lossless like any PNG; the BYTES differ from Pillow's
    (its filter heuristic and chunking), which no reader depends on (signerf/data/signerf_dataparser.py loads pixels)."""
    import struct
    import zlib

    import numpy as np

    h, w, c = u8.shape
    assert c in (1, 3) and u8.dtype == np.uint8 and h > 0 and w > 0
    flat = np.ascontiguousarray(u8).reshape(h, w * c)
    raw = np.empty((h, 1 + w * c), dtype=np.uint8)
    raw[0, 0] = 0
    raw[0, 1:] = flat[0]
    if h > 1:
        raw[1:, 0] = 2
        np.subtract(flat[1:], flat[:-1], out=raw[1:, 1:])   # modulo 256, as the format defines the filter

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if c == 1 else 2, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw, int(compress_level))) + chunk(b"IEND", b""))


class _PngHipSlot:
    """The buffers of one encode in flight for a (shape, device): the device workspace, the device file with its byte count in the 8 bytes
    before it (so ONE copy brings both) and the pinned host buffer that copy lands in.  The file's length is not known on the host when the
    copy is enqueued, so the copy is of the whole capacity (``sn_png_max_file_bytes``: a little more than the raw pixels); the file is the
    slice that is kept."""

    def __init__(self, h: int, w: int, c: int, device: torch.device):
        lib = _lib.load()
        self.shape, self.device = (h, w, c), device
        self.capacity = int(lib.sn_png_max_file_bytes(h, w, c))
        ws = int(lib.sn_png_workspace_bytes(h, w, c))
        if self.capacity == 0 or ws == 0:
            raise ValueError(f"encode_png_hip: a [{h},{w},{c}] image is not encodable (1 or 3 channels, sides in 1..8192)")
        self.workspace = torch.empty(ws, dtype=torch.uint8, device=device)
        self.out = torch.empty(8 + self.capacity, dtype=torch.uint8, device=device)
        self.host = torch.empty(8 + self.capacity, dtype=torch.uint8, pin_memory=True)
        self.done = torch.cuda.Event()

    def enqueue(self, u8: Tensor) -> None:
        """Encode + the copy to the host, on the current stream; returns without waiting."""
        lib = _lib.load()
        h, w, c = self.shape
        base = self.out.data_ptr()
        _lib.check(lib.sn_png_encode(_lib.ptr(u8), h, w, c, self.workspace.data_ptr(), self.workspace.numel(), base + 8, self.capacity, base,
                                     _lib.current_stream()), None, "sn_png_encode")
        self.host.copy_(self.out, non_blocking=True)
        self.done.record()
        self.image = u8   # alive until the kernels have read it

    def finish(self) -> bytes:
        """The one synchronisation: waits for the copy, returns the file."""
        self.done.synchronize()
        self.image = None
        n = int(self.host[:8].view(torch.int64).item())
        assert 0 < n <= self.capacity, n
        return self.host[8:8 + n].numpy().tobytes()


_png_hip_slots: Dict[Tuple[int, int, int, int], List[_PngHipSlot]] = {}
_png_hip_lock = threading.Lock()


def _png_hip_acquire(u8: Tensor) -> _PngHipSlot:
    h, w, c = (int(x) for x in u8.shape)
    key = (h, w, c, u8.device.index if u8.device.index is not None else torch.cuda.current_device())
    with _png_hip_lock:
        free = _png_hip_slots.setdefault(key, [])
        if free:
            return free.pop()
    return _PngHipSlot(h, w, c, u8.device)


def _png_hip_release(slot: _PngHipSlot) -> None:
    h, w, c = slot.shape
    with _png_hip_lock:
        free = _png_hip_slots.setdefault((h, w, c, slot.device.index if slot.device.index is not None else torch.cuda.current_device()), [])
        if len(free) < 16:   # what is kept between calls; an encode in flight beyond it allocates
            free.append(slot)


def _png_hip_enqueue(u8: Tensor) -> _PngHipSlot:
    if not (isinstance(u8, Tensor) and u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() == 3 and u8.shape[2] in (1, 3)):
        raise ValueError("encode_png_hip: a uint8 [H,W,1] or [H,W,3] tensor on the GPU is expected")
    u8 = u8.contiguous()
    slot = _png_hip_acquire(u8)
    with torch.cuda.device(u8.device):
        slot.enqueue(u8)
    return slot


def encode_png_hip(u8: Tensor) -> bytes:
    """The PNG file of a device uint8 [H,W,1] (greyscale) or [H,W,3] (RGB) tensor, encoded on the GPU (include/signerf_hip_png.h): the
    pixels ``encode_png`` stores, in a file whose bytes depend on (pixels, shape) alone.  Workspace and pinned host buffer are cached per
    (shape, device); one device-to-host copy (of the file buffer's whole capacity: the length arrives with it) and one synchronisation per
    image.  There are no compression levels."""
    slot = _png_hip_enqueue(u8)
    try:
        return slot.finish()
    finally:
        _png_hip_release(slot)


class GeneratedDataset:
    """Directory + transforms.json writer with the reference's layout and keys."""

    SUBDIRS = ("images", "masks", "conditions", "rendered", "originals")

    def __init__(self, path: Union[str, Path], dataset_name: str, downscale_factor: int = 2, write_images: bool = True, save_workers: int = 0,
                 png_compress_level: Optional[int] = None, png_encoder: str = "native"):
        """write_images=False: directories and transforms.json only (the bench's "PNG writes off" leg).  save_workers > 0: PNG encoding
        and the file writes run on that many host threads (zlib releases the GIL) while the caller goes on to the next view; the
        bytes of a file do not depend on it.  ``flush()`` waits for them.  png_compress_level: None = the reference's call
        (``Image.save(path)``, zlib level 6); 1 encodes ~2.3x faster into ~15 % larger files holding the same pixels.
        png_encoder: "native" = ``encode_png`` above (same pixels, encodes in parallel on the pool); "pil" = the reference's literal call;
        "hip" = ``encode_png_hip``: the GPU encodes, the pool (or the caller) only waits for the file and writes it.  It has no levels."""
        if png_encoder not in ("native", "pil", "hip"):
            raise ValueError(f"png_encoder={png_encoder!r}: 'native', 'pil' or 'hip' expected")
        if png_encoder == "hip" and png_compress_level is not None:
            raise ValueError("png_encoder='hip' has no compression levels: leave png_compress_level at None")
        self.png_encoder = png_encoder
        self.png_compress_level = png_compress_level
        self.dataset_path = Path(path) / dataset_name
        self.downscale_factor = downscale_factor
        self.write_images = write_images
        self.dirs: Dict[str, Path] = {}
        self._pool = None
        self._png_streams: Dict[int, List] = {}   # device index -> side streams of the "hip" encoder
        self._png_stream_next = 0
        self._pending: List = []
        # at most this many encodes queued or running: the host copies of a view's 8 PNGs must not pile up when encoding is slower than
        # the loop; a failed write surfaces at the next save instead of at the end
        self._max_pending = 16 * max(1, save_workers)
        if save_workers > 0:
            from concurrent.futures import ThreadPoolExecutor

            self._pool = ThreadPoolExecutor(max_workers=save_workers)

    def close(self) -> None:
        """Waits for the pending writes and releases the worker threads (idempotent; also runs when the object is collected)."""
        pool, self._pool = self._pool, None
        try:
            self.flush()
        finally:
            if pool is not None:
                pool.shutdown(wait=True)

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover  (interpreter shutdown)
            pass

    def init_directory(self) -> None:
        """datasetgenerator.py:146-175 (config.yml is written by DatasetGenerator.init_directory)."""
        self.dataset_path.mkdir(parents=True, exist_ok=True)
        for name in self.SUBDIRS:
            for key, d in ((name, self.dataset_path / name), (f"{name}_scaled", self.dataset_path / f"{name}_{self.downscale_factor}")):
                d.mkdir(parents=True, exist_ok=True)
                self.dirs[key] = d
        self.dirs["references"] = self.dataset_path / "references"
        self.dirs["references"].mkdir(parents=True, exist_ok=True)
        self.transforms_path = self.dataset_path / "transforms.json"

    def save_image(self, tensor: Tensor, path: Path) -> None:
        """``tensor_to_image(tensor).save(path)``: the truncating uint8 cast on the GPU, one device-to-host copy of the bytes, PNG
        encoding on the host (in the pool when there is one); with png_encoder="hip" the encoding is on the GPU too and the copy
        brings the file buffer."""
        if not self.write_images:
            return
        from PIL import Image

        assert len(tensor.shape) == 3 and tensor.shape[2] in (1, 3), "Tensor must be of shape (H, W, 1) or (H, W, 3)"
        if self.png_encoder == "hip":
            # Nothing waits here.  The cast runs on the current stream, so the caller's tensor is read in stream order.  The encode of one
            # image is a few hundred workgroups of one wave, far from filling the GPU, so encode + copy of consecutive saves (a view's
            # eight files) go round a few side streams, each behind the cast, and overlap one another and the next view's work.  The
            # uint8 image is held until the file has arrived.
            with torch.cuda.device(tensor.device):
                u8 = tensor_to_uint8(tensor)
                side = self._png_stream(tensor.device)
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    slot = _png_hip_enqueue(u8)

            def write_file():
                try:
                    data = slot.finish()
                finally:
                    _png_hip_release(slot)
                with open(path, "wb") as f:
                    f.write(data)

            # an encode in flight holds the uint8 image, a workspace, a device file and a pinned buffer, each of the image's size: few at a time
            self._submit(write_file, limit=min(self._max_pending, 16))
            return
        u8 = tensor_to_uint8(tensor).cpu().numpy()

        kw = {} if self.png_compress_level is None else {"compress_level": int(self.png_compress_level)}
        native = self.png_encoder == "native"
        level = 6 if self.png_compress_level is None else int(self.png_compress_level)

        def write():
            if native:
                data = encode_png(u8, level)
                with open(path, "wb") as f:
                    f.write(data)
            else:
                (Image.fromarray(u8.squeeze(), "L") if u8.shape[2] == 1 else Image.fromarray(u8)).save(path, **kw)

        self._submit(write)

    def _png_stream(self, device: torch.device) -> "torch.cuda.Stream":
        """The next of the device's four side streams (made at the device's first save)."""
        index = device.index if device.index is not None else torch.cuda.current_device()
        streams = self._png_streams.get(index)
        if streams is None:
            streams = self._png_streams[index] = [torch.cuda.Stream(torch.device("cuda", index)) for _ in range(4)]
        self._png_stream_next = (self._png_stream_next + 1) % len(streams)
        return streams[self._png_stream_next]

    def _submit(self, write, limit: Optional[int] = None) -> None:
        if self._pool is None:
            write()
        else:
            while len(self._pending) >= (self._max_pending if limit is None else limit):
                self._pending.pop(0).result()
            self._pending.append(self._pool.submit(write))

    def flush(self) -> None:
        pending, self._pending = self._pending, []
        for f in pending:
            f.result()

    @staticmethod
    def new_transforms(original_transform_matrix: Tensor, original_scale_factor: float, is_synthetic: bool = False,
                       is_combined: bool = False) -> Dict[str, Any]:
        """datasetgenerator.py:286-295."""
        return {"camera_model": "OPENCV", "orientation_override": "none", "method": "SIGNeRF", "is_synthetic": is_synthetic,
                "is_combined": is_combined, "frames": [],
                "original_transform_matrix": original_transform_matrix.cpu().numpy().tolist(),
                "original_scale_factor": original_scale_factor}

    def save_generated_images(self, idx: int, images: Dict[str, Tensor], camera, current_transforms: Dict[str, Any],
                              is_original: bool = False) -> Dict[str, Any]:
        """datasetgenerator.py:398-468: PNGs by key + one frame appended to the transforms."""
        def save(key: str, directory: str, stem: str):
            if key in images:
                self.save_image(images[key], self.dirs[directory] / f"{stem}_{idx}.png")

        save("edited", "images", "image")
        save("render", "originals" if is_original else "rendered", "image")
        save("mask", "masks", "mask")
        save("condition", "conditions", "condition")
        save("edited_scaled", "images_scaled", "image")
        save("render_scaled", "rendered_scaled", "image")  # the reference writes both cases to rendered_<f> (:436-440)
        save("mask_scaled", "masks_scaled", "mask")
        save("condition_scaled", "conditions_scaled", "condition")
        c2w = torch.cat([camera.camera_to_worlds.cpu(), torch.tensor([[0.0, 0.0, 0.0, 1.0]])], dim=0).numpy().tolist()
        current_transforms["frames"].append({
            "fl_x": camera.fx.item(), "fl_y": camera.fy.item(), "cx": camera.cx.item(), "cy": camera.cy.item(),
            "w": camera.width.item(), "h": camera.height.item(),
            "file_path": f"./images/image_{idx}.png",
            "_mask_path": f"./masks/mask_{idx}.png",
            "transform_matrix": c2w,  # scene space, like the reference (FIXME at datasetgenerator.py:464)
            "scene_transform_matrix": c2w,
        })
        return current_transforms

    def write_transforms(self, transforms: Dict[str, Any]) -> None:
        self.flush()
        with open(self.transforms_path, "w", encoding="utf8") as f:
            json.dump(transforms, f, indent=4)
