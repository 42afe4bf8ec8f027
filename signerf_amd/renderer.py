"""The proxy-mesh renderer of ``masking_mode="shape"`` and of ``combine_shape_with_depth`` (/root/reference/signerf/renderer/renderer.py).

The reference loads the mesh with trimesh, places it with ``pose = [R . S | position]`` and renders it with pyrender on OpenGL / EGL,
one offscreen renderer and one host read-back per view.  Here the mesh is parsed once (``load_obj``), uploaded once per device
(``Renderer.setup``), and every view is one call of ``sn_mesh_raster_depth``: a z-depth image on the GPU, sampled at the NeRF's pixel
centres (DESIGN.md "Shape masking mode" lists what differs from pyrender's multisampled 24-bit depth buffer).  ``render_camera`` returns
``(None, depth)``; with ``with_color=True`` it returns ``(color, depth)`` from one call of ``sn_mesh_raster_color``, the colour shaded as
pyrender shades a mesh under the reference's ambient-only light (``shade_defaults``; the constants are UNPINNED).

That raster is a pinhole, as pyrender's camera is, whatever lens the NeRF's camera has.  ``RendererConfig.lens = "camera"`` draws the mesh
along the camera's own rays instead (``sn_mesh_cast_rays``; DESIGN.md "Lens-aware proxy mesh"): a bounding-volume hierarchy over the posed
mesh is built once in ``setup`` (``build_accel``), uploaded once per device, and every view is one ray-cast launch.
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
    """carried for config parity and not applied, as in the reference (which stores it and never uses it): the colour image is shaded
    with the mesh's own material (``shade_defaults``)"""
    object_path: str = field(default_factory=lambda: "models/bunny.obj")
    cull_back_faces: bool = True
    """pyrender draws a mesh without a double-sided material with GL_BACK culling; False draws both sides"""
    lens: str = "pinhole"
    """not in the reference.  "pinhole": the mesh is rasterised through an ideal pinhole with the camera's fx, fy, cx, cy, as pyrender
    draws it -- distortion and camera type are ignored.  "camera": the mesh is drawn along the camera's own rays (OPENCV distortion,
    FISHEYE, EQUIRECTANGULAR), so that it lines up with the NeRF image of the same camera"""


LENSES = ("pinhole", "camera")


def load_obj(path, with_colors: bool = False):
    """Wavefront OBJ -> (vertices [V,3] float32, triangles [F,3] int32).  ``v x y z [r g b]``; ``f`` with ``a``, ``a/b``, ``a//c`` or
    ``a/b/c`` corners, 1-based or negative (relative) indices, polygons split into triangle fans.  ``vt vn vp o g s l usemtl mtllib`` and
    comments are ignored.  Raises ``ValueError`` / ``FileNotFoundError`` with the file and line for anything else.

    ``with_colors=True``: -> (vertices, triangles, colors), colors [V,4] uint8 RGBA (alpha 255) from ``v x y z r g b``, or None when no
    vertex carries a colour.  Colours within [0, 1] are quantised as ``np.round(c * 255)``; a file with any component above 1 is read as
    0..255 values.  A file where only some vertices carry a colour raises ``ValueError`` with the file and line."""
    p = Path(path)
    if p.suffix.lower() != ".obj":
        raise ValueError(f"{p}: not an .obj file (the shape masking mode reads Wavefront OBJ meshes only)")
    if not p.is_file():
        raise FileNotFoundError(f"{p}: mesh file not found")
    verts: List[Tuple[float, float, float]] = []
    tris: List[Tuple[int, int, int]] = []
    colors: List[Tuple[float, float, float]] = []
    first_v: Optional[Tuple[int, bool]] = None   # (line, has a colour) of the first vertex
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
                if with_colors:
                    has = len(parts) == 7
                    if first_v is None:
                        first_v = (ln, has)
                    elif has != first_v[1]:
                        raise ValueError(f"{p}:{ln}: this vertex {'has' if has else 'has no'} colour but the first one (line {first_v[0]}) "
                                         f"{'has' if first_v[1] else 'has none'}: either every vertex carries r g b or none does")
                    if has:
                        try:
                            colors.append((float(parts[4]), float(parts[5]), float(parts[6])))
                        except ValueError as e:
                            raise ValueError(f"{p}:{ln}: bad vertex colour: {e}") from None
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
    v, f = np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    if not with_colors:
        return v, f
    if not colors:
        return v, f, None
    c = np.asarray(colors, dtype=np.float64)
    if not np.isfinite(c).all() or (c < 0).any() or (c > 255).any():
        raise ValueError(f"{p}: vertex colours must lie in [0, 1] (or 0..255)")
    if (c <= 1.0).all():
        c = c * 255.0
    rgba = np.full((c.shape[0], 4), 255, dtype=np.uint8)
    rgba[:, :3] = np.round(c).astype(np.uint8)
    return v, f, rgba


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


def _raster_args(mv, znear: float, zfar: float, cull_back_faces: bool):
    """(``SnMeshRasterOpts``, the model-view as ``c_float * 12``) of a raster call."""
    opts = _lib.SnMeshRasterOpts()
    opts.znear, opts.zfar, opts.cull_back_faces = float(znear), float(zfar), int(bool(cull_back_faces))
    return opts, (C.c_float * 12)(*np.asarray(mv, dtype=np.float64).reshape(12).tolist())


def raster_depth(vertices: Tensor, triangles: Tensor, mv, fx: float, fy: float, cx: float, cy: float, height: int, width: int,
                 znear: float = ZNEAR, zfar: float = ZFAR, cull_back_faces: bool = True, out: Optional[Tensor] = None) -> Tensor:
    """``sn_mesh_raster_depth``: vertices [V,3] fp32 / triangles [F,3] int32 on the GPU, mv: camera-from-object [3,4] (host) ->
    z-depth [H,W,1] fp32 on the GPU, 0 where the mesh is not drawn."""
    lib = _lib.load()
    dev = vertices.device
    opts, m = _raster_args(mv, znear, zfar, cull_back_faces)
    F = int(triangles.shape[0])
    with torch.cuda.device(dev):
        depth = out if out is not None else torch.empty((height, width, 1), dtype=torch.float32, device=dev)
        ws = torch.empty(max(lib.sn_mesh_workspace_bytes(F, height, width), 1), dtype=torch.uint8, device=dev)
        _lib.check(lib.sn_mesh_raster_depth(_lib.ptr(vertices), int(vertices.shape[0]), _lib.ptr(triangles), F, m, float(fx), float(fy),
                                            float(cx), float(cy), int(height), int(width), C.byref(opts), _lib.ptr(depth), ws.data_ptr(),
                                            ws.numel(), _lib.current_stream()),
                   None, "sn_mesh_raster_depth")
    return depth


# pyrender's mesh shader under the reference's Scene(ambient_light=[1, 1, 1]) with no other light, as recalled from pyrender 0.1.45 --
# UNPINNED (pyrender is not available to check against; tools/make_pyrender_fixture.py writes the fixtures that pin them):
#   linear = ambient * baseColorFactor.rgb * COLOR_0, out = clamp(pow(linear, 1 / 2.2), 0, 1) -> unorm8, the clear colour elsewhere.
PYRENDER_DEFAULT_BASE_COLOR = (0.3, 0.3, 0.3, 1.0)   # the default material of a trimesh without visuals (the bunny: no bunny1.mtl)
PYRENDER_VERTEX_COLOR_BASE_COLOR = (1.0, 1.0, 1.0, 1.0)   # the material of a mesh with vertex colours
PYRENDER_BACKGROUND = (1.0, 1.0, 1.0)   # Scene's default bg_color (white)
REFERENCE_AMBIENT = (1.0, 1.0, 1.0)     # renderer.py:130


def shade_defaults(has_vertex_colors: bool) -> Dict[str, object]:
    """The ``raster_color`` shading keywords that stand for pyrender's, for a mesh with or without vertex colours (UNPINNED)."""
    return {"base_color": PYRENDER_VERTEX_COLOR_BASE_COLOR if has_vertex_colors else PYRENDER_DEFAULT_BASE_COLOR,
            "ambient": REFERENCE_AMBIENT, "background": PYRENDER_BACKGROUND, "gamma": True}


def raster_color(vertices: Tensor, triangles: Tensor, mv, fx: float, fy: float, cx: float, cy: float, height: int, width: int,
                 vertex_colors: Optional[Tensor] = None, base_color=PYRENDER_DEFAULT_BASE_COLOR, ambient=REFERENCE_AMBIENT,
                 background=PYRENDER_BACKGROUND, gamma: bool = True, znear: float = ZNEAR, zfar: float = ZFAR, cull_back_faces: bool = True,
                 with_depth: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """``sn_mesh_raster_color``: as ``raster_depth``, plus vertex_colors [V,4] uint8 RGBA on the GPU (or None) and the shading
    (``shade_defaults``) -> (color [H,W,3] uint8, depth [H,W,1] fp32 or None) on the GPU.  The depth is bit-identical to
    ``raster_depth``'s."""
    lib = _lib.load()
    dev = vertices.device
    if vertex_colors is not None and (vertex_colors.dtype != torch.uint8 or tuple(vertex_colors.shape) != (int(vertices.shape[0]), 4)):
        raise ValueError(f"vertex_colors must be [V,4] uint8 with V = {int(vertices.shape[0])}, got {tuple(vertex_colors.shape)} "
                         f"{vertex_colors.dtype}")
    opts, m = _raster_args(mv, znear, zfar, cull_back_faces)
    shade = _lib.SnMeshShadeOpts()
    shade.base_color[:] = [float(x) for x in base_color]
    shade.ambient[:] = [float(x) for x in ambient]
    shade.background[:] = [float(x) for x in background]
    shade.gamma = int(bool(gamma))
    F = int(triangles.shape[0])
    with torch.cuda.device(dev):
        color = torch.empty((height, width, 3), dtype=torch.uint8, device=dev)
        depth = torch.empty((height, width, 1), dtype=torch.float32, device=dev) if with_depth else None
        ws = torch.empty(max(lib.sn_mesh_color_workspace_bytes(F, height, width), 1), dtype=torch.uint8, device=dev)
        vc = None if vertex_colors is None else vertex_colors.contiguous()
        _lib.check(lib.sn_mesh_raster_color(_lib.ptr(vertices), int(vertices.shape[0]), _lib.ptr(vc), _lib.ptr(triangles), F, m, float(fx),
                                            float(fy), float(cx), float(cy), int(height), int(width), C.byref(opts), C.byref(shade),
                                            _lib.ptr(depth), _lib.ptr(color), ws.data_ptr(), ws.numel(), _lib.current_stream()),
                   None, "sn_mesh_raster_color")
    return color, depth


ACCEL_LEAF_MAX = 4   # SN_RAYS_LEAF_MAX of csrc/sn_mesh_rays.h
ACCEL_MAX_DEPTH = 32  # SN_RAYS_STACK
_ACCEL_MAGIC, _ACCEL_VERSION = 0x31524D53, 1


def _accel_leaf(first: int, count: int) -> int:
    return -(1 + first * 8 + count)


def build_accel(vertices: np.ndarray, triangles: np.ndarray) -> np.ndarray:
    """The acceleration blob of ``sn_mesh_cast_rays`` (layout: csrc/sn_mesh_rays.h) for POSED vertices [V,3] float32 and triangles [F,3]
    int32 -> uint8 [sn_mesh_accel_bytes(F)].  A binary bounding-volume hierarchy, split at the median of the triangle centroids along the
    axis of their largest extent (so its depth is about log2 F), leaves of at most 4 triangles; an inner node holds the boxes of its two
    children, widened by a few ulp.  Every triangle is in exactly one leaf; one with an index outside the vertices or a non-finite corner
    is stored with all corners at the origin (never hit), as the rasteriser drops it."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    F = int(t.shape[0])
    ok = ((t >= 0) & (t < v.shape[0])).all(1)
    corners = np.zeros((F, 3, 3), dtype=np.float32)
    corners[ok] = v[t[ok]]
    corners[~np.isfinite(corners).all((1, 2))] = 0.0
    lo, hi = corners.min(1).astype(np.float64), corners.max(1).astype(np.float64)
    cen = corners.astype(np.float64).mean(1)
    order = np.arange(F)
    cap = max(F, 1)
    boxes = np.zeros((cap, 12), dtype=np.float32)
    boxes[:, 0:3] = boxes[:, 6:9] = np.inf      # an inverted box: no child
    boxes[:, 3:6] = boxes[:, 9:12] = -np.inf
    child = np.full((cap, 2), _accel_leaf(0, 0), dtype=np.int32)
    n_nodes = 1
    # (start, end, node that owns the range's box, side of it, depth); the root's two sides are the halves of everything
    if F <= ACCEL_LEAF_MAX:
        todo = [(0, F, 0, 0, 1)] if F else []
    else:
        todo = [(0, F, -1, 0, 0)]
    while todo:
        s, e, parent, side, depth = todo.pop()
        if depth > ACCEL_MAX_DEPTH:
            raise ValueError(f"the hierarchy over {F} triangles is deeper than {ACCEL_MAX_DEPTH} levels")
        idx = order[s:e]
        if parent >= 0:
            blo, bhi = lo[idx].min(0), hi[idx].max(0)
            pad = 1e-6 * max(float(np.abs(blo).max()), float(np.abs(bhi).max())) + 1e-30
            boxes[parent, 6 * side:6 * side + 3] = np.nextafter((blo - pad).astype(np.float32), np.float32(-np.inf))
            boxes[parent, 6 * side + 3:6 * side + 6] = np.nextafter((bhi + pad).astype(np.float32), np.float32(np.inf))
        if e - s <= ACCEL_LEAF_MAX:
            child[parent, side] = _accel_leaf(s, e - s)
            continue
        if parent >= 0:
            node = n_nodes
            n_nodes += 1
            child[parent, side] = node
        else:
            node = 0
        c = cen[idx]
        axis = int(np.argmax(c.max(0) - c.min(0)))
        m = (e - s) // 2
        order[s:e] = idx[np.argpartition(c[:, axis], m)]
        todo.append((s, s + m, node, 0, depth + 1))
        todo.append((s + m, e, node, 1, depth + 1))
    header = np.zeros(16, dtype=np.uint32)
    header[:4] = [_ACCEL_MAGIC, _ACCEL_VERSION, F, n_nodes]
    nodes = np.zeros((cap, 16), dtype=np.float32)
    nodes[:, :12] = boxes
    nodes[:, 12:14] = child.view(np.float32)
    recs = np.zeros((F, 12), dtype=np.float32)
    recs[:, :9] = corners[order].reshape(F, 9)
    recs[:, 9] = order.astype(np.int32).view(np.float32)
    return np.concatenate([header.view(np.uint8), nodes.reshape(-1).view(np.uint8), recs.reshape(-1).view(np.uint8)])


def cast_rays(origins: Tensor, directions: Tensor, forward, accel: Tensor, n_triangles: int, height: int, width: int,
              triangles: Optional[Tensor] = None, vertex_colors: Optional[Tensor] = None, n_vertices: int = 0, with_color: bool = False,
              base_color=PYRENDER_DEFAULT_BASE_COLOR, ambient=REFERENCE_AMBIENT, background=PYRENDER_BACKGROUND, gamma: bool = True,
              znear: float = ZNEAR, zfar: float = ZFAR, cull_back_faces: bool = True) -> Tuple[Optional[Tensor], Tensor]:
    """``sn_mesh_cast_rays``: world-space origins / directions of height * width rays (fp32, on the GPU, row-major: what ``generate_rays``
    returns), forward: the camera's viewing axis (3 host floats), accel: ``build_accel``'s blob on the GPU -> (color [H,W,3] uint8 or None,
    z-depth [H,W,1] fp32), 0 / the background where the mesh is not drawn.  with_color needs triangles [F,3] int32 on the GPU (and takes
    vertex_colors [V,4] uint8, n_vertices = V)."""
    lib = _lib.load()
    dev = accel.device
    n = int(height) * int(width)
    if origins.numel() != 3 * n or directions.numel() != 3 * n:
        raise ValueError(f"the ray bundle holds {origins.numel() // 3} origins and {directions.numel() // 3} directions, the camera has "
                         f"{height} x {width} = {n} pixels")
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    o, d = f32(origins), f32(directions)
    if with_color and triangles is None:
        raise ValueError("with_color needs the triangles")
    if vertex_colors is not None and (vertex_colors.dtype != torch.uint8 or tuple(vertex_colors.shape) != (int(n_vertices), 4)):
        raise ValueError(f"vertex_colors must be [V,4] uint8 with V = {int(n_vertices)}, got {tuple(vertex_colors.shape)} {vertex_colors.dtype}")
    opts = _lib.SnMeshRaysOpts()
    opts.znear, opts.zfar, opts.cull_back_faces = float(znear), float(zfar), int(bool(cull_back_faces))
    shade = _lib.SnMeshShadeOpts()
    shade.base_color[:] = [float(x) for x in base_color]
    shade.ambient[:] = [float(x) for x in ambient]
    shade.background[:] = [float(x) for x in background]
    shade.gamma = int(bool(gamma))
    fwd = (C.c_float * 3)(*[float(x) for x in forward])
    with torch.cuda.device(dev):
        depth = torch.empty((height, width, 1), dtype=torch.float32, device=dev)
        color = torch.empty((height, width, 3), dtype=torch.uint8, device=dev) if with_color else None
        vc = None if vertex_colors is None else vertex_colors.contiguous()
        _lib.check(lib.sn_mesh_cast_rays(_lib.ptr(o), _lib.ptr(d), int(height), int(width), fwd, _lib.ptr(accel), accel.numel(),
                                         _lib.ptr(triangles), int(n_triangles), _lib.ptr(vc), int(n_vertices), C.byref(opts),
                                         C.byref(shade) if with_color else None, _lib.ptr(depth), _lib.ptr(color), _lib.current_stream()),
                   None, "sn_mesh_cast_rays")
    return color, depth


class Renderer:
    """``Renderer`` of the reference (renderer.py:43-196): the depth it feeds the shape masking mode and the colour + depth that
    ``combine_shape_with_depth`` pastes into the aabb condition."""

    def __init__(self, config: RendererConfig, device="cuda") -> None:
        if config.lens not in LENSES:
            raise ValueError(f"RendererConfig.lens = {config.lens!r}: must be one of {', '.join(LENSES)}")
        self.config = config
        self.device = device
        self.position, self.rotation, self.scale, self.color = config.position, config.rotation, config.scale, config.color
        self.object_path = config.object_path
        self.pose: Optional[np.ndarray] = None
        self._host_mesh: Optional[Tuple[np.ndarray, np.ndarray]] = None
        self._host_colors: Optional[Tuple[Optional[np.ndarray]]] = None   # ([V,4] uint8 vertex colours or None,) once read
        self._uploaded: Dict[str, Tuple[Tensor, Tensor]] = {}
        self._uploaded_colors: Dict[str, Optional[Tensor]] = {}
        self._host_accel: Optional[np.ndarray] = None   # lens == "camera": build_accel's blob of the posed mesh
        self._uploaded_accel: Dict[str, Tensor] = {}

    def setup(self) -> None:
        """Parse the mesh and compute its pose (renderer.py:64-121).  Unlike the reference, a missing or non-OBJ file raises here.
        With ``lens="camera"`` the acceleration structure of the posed mesh is built here too, once."""
        self._host_mesh = load_obj(self.object_path)
        self.pose = object_pose(self.config)
        self._host_colors, self._uploaded, self._uploaded_colors = None, {}, {}
        self._host_accel, self._uploaded_accel = None, {}
        if self.config.lens == "camera":
            v, f = self._host_mesh
            world = (v.astype(np.float64) @ self.pose[:3, :3].T + self.pose[:3, 3]).astype(np.float32)
            self._host_accel = build_accel(world, f)

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

    def colors_on(self, device) -> Optional[Tensor]:
        """The vertex colours [V,4] uint8 on `device`, or None when the mesh has none.  The file's colours are read the first time a
        colour image is rendered (so a mesh whose colours are malformed still renders its depth, as before), uploaded once per device."""
        verts, _ = self.mesh_on(device)
        if self._host_colors is None:
            self._host_colors = (load_obj(self.object_path, with_colors=True)[2],)
        key = str(verts.device)
        if key not in self._uploaded_colors:
            c = self._host_colors[0]
            self._uploaded_colors[key] = None if c is None else torch.from_numpy(c).to(verts.device)
        return self._uploaded_colors[key]

    def accel_on(self, device) -> Tensor:
        """``build_accel``'s blob on `device` (``lens="camera"``), uploaded the first time a view of that device is rendered."""
        verts, _ = self.mesh_on(device)
        if self._host_accel is None:
            raise RuntimeError('Renderer.setup() built no acceleration structure: RendererConfig.lens was not "camera" then')
        key = str(verts.device)
        if key not in self._uploaded_accel:
            self._uploaded_accel[key] = torch.from_numpy(self._host_accel).to(verts.device)
        return self._uploaded_accel[key]

    def render_camera(self, camera, with_color: bool = False, ray_bundle=None) -> Tuple[Optional[Tensor], Tensor]:
        """-> (None, depth [H,W,1] fp32 on the camera's device); with_color: (color [H,W,3] uint8, depth), shaded as pyrender shades the
        mesh under the reference's ambient light (``shade_defaults``).  Intrinsics and pose come from the camera's host mirror (no device
        sync).  ``lens="pinhole"`` (the default): distortion and camera type are ignored, as pyrender's IntrinsicsCamera ignores them, and
        so is `ray_bundle`.  ``lens="camera"``: the mesh along the camera's rays -- `ray_bundle` (the H x W bundle the caller has already
        generated for this camera) or, without one, ``generate_rays(camera_indices=0)``; a bundle of another size raises ValueError."""
        from .cameras import Cameras

        cam = Cameras.from_cameras(camera)
        host = cam._host.reshape(-1, cam._host.shape[-1])[0].tolist()  # pylint: disable=protected-access
        fx, fy, cx, cy = host[12], host[13], host[14], host[15]
        W, H = int(host[16]), int(host[17])
        dev = cam.device if cam.device.type == "cuda" else torch.device(self.device)
        verts, tris = self.mesh_on(dev)
        if self.config.lens == "camera":
            accel = self.accel_on(dev)
            if ray_bundle is None:
                ray_bundle = (cam if cam.device.type == "cuda" else cam.to(dev)).generate_rays(camera_indices=0)
            vc = self.colors_on(dev) if with_color else None
            forward = (-host[2], -host[6], -host[10])   # a nerfstudio camera looks down its -z axis
            return cast_rays(ray_bundle.origins, ray_bundle.directions, forward, accel, int(tris.shape[0]), H, W, tris, vc, int(verts.shape[0]),
                             with_color, znear=ZNEAR, zfar=ZFAR, cull_back_faces=self.config.cull_back_faces, **shade_defaults(vc is not None))
        mv = model_view(host[:12], self.pose)
        if not with_color:
            return None, raster_depth(verts, tris, mv, fx, fy, cx, cy, H, W, ZNEAR, ZFAR, self.config.cull_back_faces)
        vc = self.colors_on(dev)
        return raster_color(verts, tris, mv, fx, fy, cx, cy, H, W, vc, znear=ZNEAR, zfar=ZFAR, cull_back_faces=self.config.cull_back_faces,
                            **shade_defaults(vc is not None))
