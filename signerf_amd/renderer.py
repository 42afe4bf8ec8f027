"""The proxy-mesh depth renderer of ``masking_mode="shape"`` (/root/reference/signerf/renderer/renderer.py).

The reference loads the mesh with trimesh, places it with ``pose = [R . S | position]`` and renders it with pyrender on OpenGL / EGL,
one offscreen renderer and one host read-back per view.  Here the mesh is parsed once (``load_obj``), uploaded once per device
(``Renderer.setup``), and every view is one call of ``sn_mesh_raster_depth``: a z-depth image on the GPU, sampled at the NeRF's pixel
centres (DESIGN.md "Shape masking mode" lists what differs from pyrender's multisampled 24-bit depth buffer).  The colour image is not
produced: ``render_camera`` returns ``(None, depth)``.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib

NERFSTUDIO_BLENDER_SCALE_RATIO: float = 10.0
ZNEAR, ZFAR = 1e-4, 10.0  # pyrender.IntrinsicsCamera(znear=0.0001, zfar=10) in the reference


@dataclass
class RendererConfig:
    """``RendererConfig`` of the reference (renderer.py:24-40): the same fields and defaults."""

    position: List[float] = field(default_factory=lambda: [0.0, 0.0, 0.0])
    rotation: List[float] = field(default_factory=lambda: [0, 0, 0])
    """degrees about x, y, z; applied as Rz . Ry . Rx"""
    scale: List[float] = field(default_factory=lambda: [0.1, 0.1, 0.1])
    color: List[float] = field(default_factory=lambda: [0.0, 0.0, 0.0, 1.0])
    """carried for config parity: the colour image is not rendered"""
    object_path: str = field(default_factory=lambda: "models/bunny.obj")
    cull_back_faces: bool = True
    """pyrender draws a mesh without a double-sided material with GL_BACK culling; False draws both sides"""


def load_obj(path) -> Tuple[np.ndarray, np.ndarray]:
    """Wavefront OBJ -> (vertices [V,3] float32, triangles [F,3] int32).  ``v x y z [r g b]``; ``f`` with ``a``, ``a/b``, ``a//c`` or
    ``a/b/c`` corners, 1-based or negative (relative) indices, polygons split into triangle fans.  ``vt vn vp o g s l usemtl mtllib`` and
    comments are ignored.  Raises ``ValueError`` / ``FileNotFoundError`` with the file and line for anything else."""
    p = Path(path)
    if p.suffix.lower() != ".obj":
        raise ValueError(f"{p}: not an .obj file (the shape masking mode reads Wavefront OBJ meshes only)")
    if not p.is_file():
        raise FileNotFoundError(f"{p}: mesh file not found")
    verts: List[Tuple[float, float, float]] = []
    tris: List[Tuple[int, int, int]] = []
    with open(p, "r", encoding="utf8", errors="replace") as fh:
        for ln, line in enumerate(fh, 1):
            parts = line.split("#", 1)[0].split()
            if not parts:
                continue
            key = parts[0]
            if key == "v":
                if len(parts) < 4:
                    raise ValueError(f"{p}:{ln}: a vertex needs three coordinates")
                try:
                    verts.append((float(parts[1]), float(parts[2]), float(parts[3])))
                except ValueError as e:
                    raise ValueError(f"{p}:{ln}: bad vertex: {e}") from None
            elif key == "f":
                if len(parts) < 4:
                    raise ValueError(f"{p}:{ln}: a face needs at least three corners")
                idx = []
                for c in parts[1:]:
                    try:
                        k = int(c.split("/", 1)[0])
                    except ValueError:
                        raise ValueError(f"{p}:{ln}: bad face corner {c!r}") from None
                    if k > 0:
                        k -= 1
                    elif k < 0:
                        k += len(verts)   # relative to the vertices read so far
                    else:
                        raise ValueError(f"{p}:{ln}: face index 0 (OBJ indices start at 1)")
                    if not 0 <= k < len(verts):
                        raise ValueError(f"{p}:{ln}: face index {c!r} is outside the {len(verts)} vertices defined so far")
                    idx.append(k)
                for i in range(1, len(idx) - 1):
                    tris.append((idx[0], idx[i], idx[i + 1]))
            # vt, vn, vp, o, g, s, l, usemtl, mtllib, ...: not geometry this renderer draws
    if not tris:
        raise ValueError(f"{p}: no faces")
    return np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(tris, dtype=np.int32).reshape(-1, 3)


def object_pose(cfg: RendererConfig) -> np.ndarray:
    """The mesh's object-to-world pose [4,4] float64 (renderer.py:81-121): R = Rz . Ry . Rx (degrees), S = diag(scale * 10), [R . S | position].
    (The reference applies its Blender -> OpenGL ``convert`` matrix to both this pose and the camera pose: it cancels in the view.)"""
    rx, ry, rz = (math.radians(a) for a in cfg.rotation)
    Rx = np.array([[1, 0, 0], [0, math.cos(rx), -math.sin(rx)], [0, math.sin(rx), math.cos(rx)]])
    Ry = np.array([[math.cos(ry), 0, math.sin(ry)], [0, 1, 0], [-math.sin(ry), 0, math.cos(ry)]])
    Rz = np.array([[math.cos(rz), -math.sin(rz), 0], [math.sin(rz), math.cos(rz), 0], [0, 0, 1]])
    R = Rz @ (Ry @ Rx)
    S = np.diag([s * NERFSTUDIO_BLENDER_SCALE_RATIO for s in cfg.scale])
    pose = np.zeros((4, 4))
    pose[0:3, 0:3] = R @ S
    pose[:, 3] = list(cfg.position) + [1]
    return pose


def model_view(c2w, pose: np.ndarray) -> np.ndarray:
    """Camera-from-object [3,4] float64: inv(c2w as 4x4) @ pose (the full inverse, as pyrender inverts the camera node's matrix)."""
    m = np.eye(4)
    m[:3, :4] = np.asarray(c2w, dtype=np.float64).reshape(3, 4)
    return (np.linalg.inv(m) @ pose)[:3]


def raster_depth(vertices: Tensor, triangles: Tensor, mv, fx: float, fy: float, cx: float, cy: float, height: int, width: int,
                 znear: float = ZNEAR, zfar: float = ZFAR, cull_back_faces: bool = True, out: Optional[Tensor] = None) -> Tensor:
    """``sn_mesh_raster_depth``: vertices [V,3] fp32 / triangles [F,3] int32 on the GPU, mv: camera-from-object [3,4] (host) ->
    z-depth [H,W,1] fp32 on the GPU, 0 where the mesh is not drawn."""
    lib = _lib.load()
    dev = vertices.device
    opts = _lib.SnMeshRasterOpts()
    opts.znear, opts.zfar, opts.cull_back_faces = float(znear), float(zfar), int(bool(cull_back_faces))
    m = (C.c_float * 12)(*np.asarray(mv, dtype=np.float64).reshape(12).tolist())
    F = int(triangles.shape[0])
    with torch.cuda.device(dev):
        depth = out if out is not None else torch.empty((height, width, 1), dtype=torch.float32, device=dev)
        ws = torch.empty(max(lib.sn_mesh_workspace_bytes(F, height, width), 1), dtype=torch.uint8, device=dev)
        _lib.check(lib.sn_mesh_raster_depth(_lib.ptr(vertices), int(vertices.shape[0]), _lib.ptr(triangles), F, m, float(fx), float(fy),
                                            float(cx), float(cy), int(height), int(width), C.byref(opts), _lib.ptr(depth), ws.data_ptr(),
                                            ws.numel(), _lib.current_stream()),
                   None, "sn_mesh_raster_depth")
    return depth


class Renderer:
    """``Renderer`` of the reference (renderer.py:43-196) for the depth it feeds the shape masking mode."""

    def __init__(self, config: RendererConfig, device="cuda") -> None:
        self.config = config
        self.device = device
        self.position, self.rotation, self.scale, self.color = config.position, config.rotation, config.scale, config.color
        self.object_path = config.object_path
        self.pose: Optional[np.ndarray] = None
        self._host_mesh: Optional[Tuple[np.ndarray, np.ndarray]] = None
        self._uploaded: Dict[str, Tuple[Tensor, Tensor]] = {}

    def setup(self) -> None:
        """Parse the mesh and compute its pose (renderer.py:64-121).  Unlike the reference, a missing or non-OBJ file raises here."""
        self._host_mesh = load_obj(self.object_path)
        self.pose = object_pose(self.config)
        self._uploaded = {}

    @property
    def num_triangles(self) -> int:
        return 0 if self._host_mesh is None else int(self._host_mesh[1].shape[0])

    def mesh_on(self, device) -> Tuple[Tensor, Tensor]:
        """(vertices, triangles) on `device`, uploaded the first time a view of that device is rendered."""
        if self._host_mesh is None:
            raise RuntimeError("Renderer.setup() has not been called")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = str(dev)
        if key not in self._uploaded:
            v, f = self._host_mesh
            self._uploaded[key] = (torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))
        return self._uploaded[key]

    def render_camera(self, camera) -> Tuple[None, Tensor]:
        """-> (None, depth [H,W,1] fp32 on the camera's device).  Intrinsics and pose come from the camera's host mirror (no device
        sync); pinhole only -- distortion and camera type are ignored, as pyrender's IntrinsicsCamera ignores them."""
        from .cameras import Cameras

        cam = Cameras.from_cameras(camera)
        host = cam._host.reshape(-1, cam._host.shape[-1])[0].tolist()  # pylint: disable=protected-access
        fx, fy, cx, cy = host[12], host[13], host[14], host[15]
        W, H = int(host[16]), int(host[17])
        dev = cam.device if cam.device.type == "cuda" else torch.device(self.device)
        verts, tris = self.mesh_on(dev)
        mv = model_view(host[:12], self.pose)
        return None, raster_depth(verts, tris, mv, fx, fy, cx, cy, H, W, ZNEAR, ZFAR, self.config.cull_back_faces)
